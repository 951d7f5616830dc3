"""Host-pointer placed and spanned scores through the chunk pipeline: wall time of a call beside the host-side phases
describe() reports for it (host_gather_ms: gathering and packing, host_wait_ms: blocked on the device, host_drain_ms: copy-out).

  python tools/host_pipeline_bench.py [--root CHECKOUT] [--label NAME] [--entry placed,span] [--pairs 262144] [--calls 15] [--threads 16]

One process, one engine per entry point of --entry: a warm-up call, then --calls timed calls (the calls are synchronous: host arrays in,
host records out); one RESULT line per entry point with every call's figures, the medians and a checksum of the records.
--root: import the package (and with it the library) of another checkout of this repository -- a build of the parent commit
next to this tree's, run alternately, shows the run-to-run spread of one library beside the difference between the two.
150 x 500 at the default chunk size is 65,536 pairs a chunk: 262,144 pairs are four chunks over the four staging slots.
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--entry", default="placed,span")
    ap.add_argument("--calls", type=int, default=15)
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from versalignlib_amd import hipkernel, synth

    R, F, block = 150, 500, 4096
    reads, refs = synth.make_pairs(block, R, F, seed=7, sub_rate=0.1, indel_rate=0.01)
    reps = (args.pairs + block - 1) // block
    reads, refs = np.tile(reads, (reps, 1))[:args.pairs].copy(), np.tile(refs, (reps, 1))[:args.pairs].copy()
    sc = hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)
    for name in args.entry.split(","):
        eng = hipkernel.Engine(R, F, sc)
        call = eng.score_placed_host if name == "placed" else eng.score_span_host
        out = call(0, reads, refs, threads=args.threads)
        calls = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            out = call(0, reads, refs, threads=args.threads)
            wall = (time.perf_counter() - t0) * 1e3
            d = eng.describe(0, args.pairs)
            calls.append({"wall_ms": round(wall, 3), "gather_ms": d["host_gather_ms"], "wait_ms": d["host_wait_ms"], "drain_ms": d["host_drain_ms"]})
        rec = {"label": args.label, "call": "score_%s_host" % name, "pairs": args.pairs, "ran": d["ran_span" if name == "span" else "ran_placed"],
               "packed_classes": d["packed_classes"], "direct_call": d["direct_call"],
               "median": {k: round(statistics.median(c[k] for c in calls), 3) for k in calls[0]}, "calls": calls,
               "checksum": int(sum(int(out[k].astype(np.int64).sum()) for k in out.dtype.names))}
        eng.close()
        print("RESULT " + json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
