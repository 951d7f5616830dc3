"""What placed Smith-Waterman scores cost: score_device on int16 cells, score_device at its default, score_placed_device and
align_cigar_device in one process, on the bench batch (1,048,576 pairs of 150 x 500) and on 10 kbp x 10 kbp (4,096 pairs, where
placed scores take the row strips; align_cigar_device with and without trace_checkpoints), SW linear 2 / -1 / -3 and SW affine
open -5, extend -1.

  python -m tools.placed_bench [--short-pairs 1048576] [--long-pairs 4096] [--reps 7] [--skip-long]

Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the
median and the minimum of --reps launches are printed, then a JSON summary.  TCUPS = pairs x R x F / time.
"""
import argparse
import json
import statistics

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


def leg(name, R, F, n, scoring, reps, block, long_read):
    reads, refs = _batch(n, R, F, 7, block)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    cells = float(n) * R * F
    results = []

    def report(call, med, best, ran):
        results.append({"leg": name, "call": call, "ms_median": round(med, 3), "ms_min": round(best, 3), "tcups": round(cells / med / 1e9, 3), "ran": ran})
        print("%-22s %-34s %10.3f ms (min %10.3f)  %7.3f TCUPS  %s" % (name, call, med, best, cells / med / 1e9, ran), flush=True)

    scores = torch.empty(n, dtype=torch.int16, device="cuda")
    for half in (0, 1):
        eng = hipkernel.Engine(R, F, scoring)
        eng.set_half_float_cells(half)
        med, best = _timed(lambda: eng.score_device(0, d_reads, d_refs, scores=scores), reps)
        report("score_device half_float_cells=%d" % half, med, best, eng.describe(0, n)["ran_score_cells"])
        eng.close()
    eng = hipkernel.Engine(R, F, scoring)
    placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
    med, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), reps)
    report("score_placed_device", med, best, eng.describe(0, n)["ran_placed"])
    same = bool((placed[:, 0].to(torch.int16) == scores).all())
    eng.close()
    stride = 4096 if long_read else 64
    for ckpt in ((0, 1) if long_read else (0,)):
        eng = hipkernel.Engine(R, F, scoring)
        eng.set_trace_checkpoints(ckpt)
        recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
        ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
        med, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=stride, out=(recs, ops)), max(2, reps // 2) if long_read else reps)
        report("align_cigar_device ckpt=%d" % ckpt, med, best, eng.describe(0, n)["ran_align_fill"])
        same = same and bool((recs[:, 1] == placed[:, 1]).all()) and bool((recs[:, 3] == placed[:, 2]).all())
        del recs, ops
        eng.close()
    print("%-22s placed score == score_device and placed ends == cigar record ends: %s" % (name, same), flush=True)
    results.append({"leg": name, "consistent": same})
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-pairs", type=int, default=1 << 20)
    ap.add_argument("--long-pairs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-long", action="store_true")
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(2, -1, -3, -3)
    affine = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)
    out = []
    for name, sc in (("SW linear", linear), ("SW affine", affine)):
        out += leg("150x500 " + name, 150, 500, args.short_pairs, sc, args.reps, 4096, False)
    if not args.skip_long:
        for name, sc in (("SW linear", linear), ("SW affine", affine)):
            out += leg("10kx10k " + name, 10000, 10000, args.long_pairs, sc, max(3, args.reps // 2), 64, True)
    print(json.dumps({"tool": "placed_bench", "results": out}))


if __name__ == "__main__":
    main()
