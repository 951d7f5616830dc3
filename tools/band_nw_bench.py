"""Time the banded NW variant (band_nw = 1) beside banded Smith-Waterman and the unbanded NW variant on the device entry points
(developer tool): scores per --score-pairs pairs, alignments (fill + walk) per --align-pairs pairs, linear and affine gaps, in one
run.  A warm-up call, then --iters event-timed calls each: the range and the median are printed, one JSON line per mode."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench
from versalignlib_amd import hipkernel


def timed(call, iters):
    call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms.sort()
    return {"ms_min": round(ms[0], 2), "ms_median": round(ms[len(ms) // 2], 2), "ms_max": round(ms[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--R", type=int, default=10000)
    ap.add_argument("--F", type=int, default=10000)
    ap.add_argument("--band", type=int, default=512)
    ap.add_argument("--score-pairs", type=int, default=32768)
    ap.add_argument("--align-pairs", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--what", default="scores,aligns")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    bench.R, bench.F = a.R, a.F
    n = max(a.score_pairs if "scores" in a.what else 0, a.align_pairs)
    reads, refs = bench.synth_on_device(n, dev, seed=2000, R=a.R, F=a.F)
    for model in ("linear", "affine"):
        sc = hipkernel.Scoring.make(2, -1, -3, -3, **(bench.AFFINE if model == "affine" else {}))
        # (opt, band, name): NW banded beside SW banded, and -- alignments -- the unbanded NW variant
        for opt, band, name in ((1, a.band, "nw_band"), (0, a.band, "sw_band"), (1, 0, "nw_unbanded")):
            eng = hipkernel.Engine(a.R, a.F, sc)
            eng.set_band_width(band)
            eng.set_band_alignments(1 if band else 0)
            eng.set_band_nw(1 if band else 0)
            if "scores" in a.what:
                r, f = reads[:a.score_pairs], refs[:a.score_pairs]
                scores = torch.empty(a.score_pairs, dtype=torch.int16, device=dev)
                t = timed(lambda: eng.score_device(opt, r, f, scores), a.iters)
                d = eng.describe(opt, a.score_pairs)
                print(json.dumps(dict({"mode": "%s_%s_score" % (name, model), "pairs": a.score_pairs, "band": band, "cells": d["ran_score_cells"],
                                       "block": [d["band_block_rows"], d["band_col_align"]], "checksum": int(scores.to(torch.int64).sum().item())}, **t)), flush=True)
            if "aligns" in a.what:
                r, f = reads[:a.align_pairs], refs[:a.align_pairs]
                rows = torch.empty((a.align_pairs, 2, a.R + a.F), dtype=torch.uint8, device=dev)
                idx = torch.empty((a.align_pairs, 4), dtype=torch.int16, device=dev)
                t = timed(lambda: eng.align_device(opt, r, f, rows, idx), a.iters)
                d = eng.describe(opt, a.align_pairs)
                print(json.dumps(dict({"mode": "%s_%s_align" % (name, model), "pairs": a.align_pairs, "band": band, "fill": d["ran_align_fill"],
                                       "ptr_bytes_per_pair": d["align_ptr_bytes_per_pair"], "start_checksum": int(idx[:, 0].to(torch.int64).sum().item())}, **t)), flush=True)
                del rows, idx
            eng.close()


if __name__ == "__main__":
    main()
