"""What the compact result format costs: align_cigar_device against align_device, align_cigar_host against align_host into
registered flat buffers (the cheapest way the rows reach a host), on synthetic batches.

  python -m tools.cigar_bench [--short-pairs 1048576] [--long-pairs 4096] [--threads 16] [--reps 5] [--skip-long] [--skip-host]

Prints one line per measurement and a JSON summary last.  Times are wall-clock around a synchronised call (median of --reps
after two warm-up calls).  `lanes` is the encoder's lane group per pair (VALIGN_HIP_DEBUG cigar_lanes; 0: the engine's choice).
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

from versalignlib_amd import hipkernel, synth


def _timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out)


def _engine(R, F, scoring, lanes=0, ckpt=0):
    if lanes:
        os.environ["VALIGN_HIP_DEBUG"] = "cigar_lanes=%d" % lanes
    else:
        os.environ.pop("VALIGN_HIP_DEBUG", None)
    eng = hipkernel.Engine(R, F, scoring)
    eng.set_trace_checkpoints(ckpt)
    return eng


def _batch(n, R, F, seed, block=4096):
    reads, refs = synth.make_pairs(min(n, block), R, F, seed=seed, sub_rate=0.1, indel_rate=0.0 if R > 2000 else 0.01)
    reps = (n + len(reads) - 1) // len(reads)
    return np.tile(reads, (reps, 1))[:n].copy(), np.tile(refs, (reps, 1))[:n].copy()


def device_leg(name, R, F, n, opt, scoring, reps, lanes_list, ckpt=0, stride=64, block=4096):
    reads, refs = _batch(n, R, F, 7, block)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    results = []
    eng = _engine(R, F, scoring, 0, ckpt)
    rows = torch.empty((n, 2, R + F), dtype=torch.uint8, device="cuda")
    idx = torch.empty((n, 4), dtype=torch.int16, device="cuda")
    med, best = _timed(lambda: eng.align_device(opt, d_reads, d_refs, rows=rows, idx=idx), reps)
    ran = eng.describe(opt, n)["ran_align_fill"]
    del rows, idx
    eng.close()
    results.append({"leg": name, "call": "align_device", "ms_median": round(med, 3), "ms_min": round(best, 3), "fill": ran})
    print("%-28s align_device              %9.3f ms (min %9.3f)  %s" % (name, med, best, ran), flush=True)
    for lanes in lanes_list:
        eng = _engine(R, F, scoring, lanes, ckpt)
        recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
        ops = torch.empty((n, stride), dtype=torch.int32, device="cuda")
        med, best = _timed(lambda: eng.align_cigar_device(opt, d_reads, d_refs, extended=True, ops_stride=stride, out=(recs, ops)), reps)
        n_ops = recs[:, 5]
        results.append({"leg": name, "call": "align_cigar_device", "lanes": lanes, "ms_median": round(med, 3), "ms_min": round(best, 3),
                        "mean_ops": round(float(n_ops.float().mean()), 2), "max_ops": int(n_ops.max()),
                        "rows_scratch_mb": round(eng.describe(opt, n)["cigar_rows_scratch_bytes"] / 1e6, 1)})
        print("%-28s align_cigar_device lanes=%-2d %9.3f ms (min %9.3f)  mean ops %.1f max %d" %
              (name, lanes, med, best, results[-1]["mean_ops"], results[-1]["max_ops"]), flush=True)
        del recs, ops
        eng.close()
    return results


def host_leg(R, F, n, opt, scoring, reps, threads):
    reads, refs = _batch(n, R, F, 7)
    eng = _engine(R, F, scoring)
    rows = np.zeros((n, 2, R + F), np.uint8)
    idx = np.zeros((n, 4), np.int16)
    hipkernel.host_register(rows)
    hipkernel.host_register(idx)
    results = []
    try:
        med, best = _timed(lambda: eng.align_host(opt, reads, refs, threads=threads, out=(rows, idx)), reps)
        d = eng.describe(opt, n)
        results.append({"leg": "host", "call": "align_host(registered)", "ms_median": round(med, 3), "ms_min": round(best, 3), "d2h_mb": d["full_row_mb"],
                        "gather_ms": d["host_gather_ms"], "wait_ms": d["host_wait_ms"], "drain_ms": d["host_drain_ms"]})
        print("host %dx%d n=%d  align_host (registered rows)   %9.3f ms (min %9.3f)  D2H %.0f MB" % (R, F, n, med, best, d["full_row_mb"]), flush=True)
    finally:
        hipkernel.host_unregister(rows)
        hipkernel.host_unregister(idx)
    del rows
    med, best = _timed(lambda: eng.align_host(opt, reads, refs, threads=threads), max(2, reps // 2))
    d = eng.describe(opt, n)
    results.append({"leg": "host", "call": "align_host(staged, packed rows)", "ms_median": round(med, 3), "ms_min": round(best, 3), "d2h_mb": d["d2h_row_mb"]})
    print("host %dx%d n=%d  align_host (staged)            %9.3f ms (min %9.3f)  D2H %.0f MB" % (R, F, n, med, best, d["d2h_row_mb"]), flush=True)
    cap = 64 * n
    box = {}

    def call():
        box["out"] = eng.align_cigar_host(opt, reads, refs, extended=True, threads=threads, ops_cap=cap)
    med, best = _timed(call, reps)
    d = eng.describe(opt, n)
    results.append({"leg": "host", "call": "align_cigar_host", "ms_median": round(med, 3), "ms_min": round(best, 3),
                    "d2h_mb": round(d["cigar_d2h_bytes"] / 1e6, 1), "gather_ms": d["host_gather_ms"], "wait_ms": d["host_wait_ms"],
                    "drain_ms": d["host_drain_ms"], "total_ops": int(box["out"][2][-1])})
    print("host %dx%d n=%d  align_cigar_host               %9.3f ms (min %9.3f)  D2H %.1f MB  gather %.1f wait %.1f drain %.1f ms (includes numpy allocation of the outputs)" %
          (R, F, n, med, best, d["cigar_d2h_bytes"] / 1e6, d["host_gather_ms"], d["host_wait_ms"], d["host_drain_ms"]), flush=True)
    eng.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--short-pairs", type=int, default=1 << 20)
    ap.add_argument("--long-pairs", type=int, default=4096)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip-long", action="store_true")
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    linear = hipkernel.Scoring.make(2, -1, -3, -3)
    affine = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)
    out = []
    out += device_leg("150x500 SW linear", 150, 500, args.short_pairs, 0, linear, args.reps, (16, 64))
    out += device_leg("150x500 NW affine", 150, 500, args.short_pairs, 1, affine, args.reps, (16, 64))
    if not args.skip_long:
        for ckpt in (0, 1):
            out += device_leg("10kx10k SW linear ckpt=%d" % ckpt, 10000, 10000, args.long_pairs, 0, linear, max(2, args.reps // 2), (64, 16),
                              ckpt=ckpt, stride=4096, block=64)
    if not args.skip_host:
        out += host_leg(150, 500, args.short_pairs, 0, linear, args.reps, args.threads)
    print(json.dumps({"tool": "cigar_bench", "results": out}))


if __name__ == "__main__":
    main()
