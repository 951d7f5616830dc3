"""What banded placed scores cost, at 10 kbp x 10 kbp under a band of 512 diagonals (SW linear 2 / -1 / -3 and SW affine open -5,
extend -1), in one run:

  sweep ......... score_device under the band (the block chain), 32,768 pairs -- on this tree's library and, with --parent-lib, on
                  a library built from the parent commit, alternating, so that the file shows the run-to-run spread of one
                  library beside the difference between the two (the score instances are meant to be the same code);
  placed ........ score_placed_device under band_placed = 1, 32,768 pairs, checked against the sweep's scores;
  align ......... align_cigar_device under band_alignments = 1, 4,096 pairs: the other way to learn where a banded alignment ends;
  strip ......... score_placed_device without a band (the row strips' forward pass), 4,096 pairs.

  python -m tools.placed_band_bench [--parent-lib PATH] [--pairs 32768] [--align-pairs 4096] [--reps 5] [--rounds 2]

Every leg is a fresh child process (one engine family per process, nothing shared but the device), run one after the other
under a time limit of its own; the first that fails ends the run.  Inputs are resident on the device; every call is timed with
events around it on one stream after two warm-up calls; the median and the minimum of --reps launches are printed, then a JSON
summary with the placed / sweep ratio beside the ratio predicted from instruction counts (PREDICTED below; DESIGN.md has the
count).  Per-pair times are what the comparison with `align` and `strip` is about: they run an eighth of the pairs.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

R = F = 10000
BAND = 512
# Predicted placed / sweep ratio from instruction counts (tools/isa_histogram.py --part main, the UNIT + SYM instances; issue
# cycles per wave at 4.3 per half-rate and 2.6 per full-rate VALU instruction).  The tool's hot loop is one step plus the event
# code: sweep 751 (linear) / 1006 (affine) cycles, placed 878 / 1133.  A step gains 15 v_lshl_or_b32 + 1 v_lshlrev_b32 (the
# keys), one compare and one select: 16 x 4.3 + 2 x 2.6 = 74 cycles; the rest of the 127 is the event's (settling the lane's
# record), which runs once per d = 17 steps.  So: between 1 + 74 / 751 and 878 / 751 (linear), 1 + 74 / 1006 and 1133 / 1006.
# (profiles/r11_placed_band.txt measured 1.284 and 1.137: the count underestimates, the linear range is missed -- kept as the
# prediction it was, so that the summary goes on showing the two side by side)
PREDICTED = {"linear": (round(1 + 74 / 751, 3), round(878 / 751, 3)), "affine": (round(1 + 74 / 1006, 3), round(1133 / 1006, 3))}


def _timed(fn, reps):
    import torch
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


def _batch(n, seed=7, block=64):
    import numpy as np
    from versalignlib_amd import synth
    reads, refs = synth.make_pairs(block, R, F, seed=seed, sub_rate=0.1, indel_rate=0.0)
    reps = (n + block - 1) // block
    return np.tile(reads, (reps, 1))[:n].copy(), np.tile(refs, (reps, 1))[:n].copy()


def _scorings():
    from versalignlib_amd import hipkernel
    return (("linear", hipkernel.Scoring.make(2, -1, -3, -3)), ("affine", hipkernel.Scoring.make(2, -1, -3, -3, -5, -1, -5, -1)))


class _SweepEngine:
    """The four entry points the sweep needs, bound by hand: the same calls on this tree's library and on one built from an
    earlier commit (which hipkernel.lib() rightly refuses to load: it lacks the newer symbols)"""

    def __init__(self, path, scoring):
        import ctypes
        self.L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        self.L.valign_hip_engine_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        self.L.valign_hip_engine_destroy.restype = None
        self.L.valign_hip_engine_destroy.argtypes = [vp]
        self.L.valign_hip_set_band_width.argtypes = [vp, ctypes.c_int]
        self.L.valign_hip_score_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        self.L.valign_hip_last_error.restype = ctypes.c_char_p
        self.h = vp()
        self._check(self.L.valign_hip_engine_create(0, R, F, ctypes.addressof(scoring), 0, 0, ctypes.byref(self.h)))
        self._check(self.L.valign_hip_set_band_width(self.h, BAND))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.valign_hip_last_error().decode(errors="replace"))

    def score(self, d_reads, d_refs, scores, stream):
        self._check(self.L.valign_hip_score_device(self.h, 0, d_reads.shape[0], d_reads.data_ptr(), d_refs.data_ptr(), scores.data_ptr(), stream))

    def close(self):
        self.L.valign_hip_engine_destroy(self.h)


def child(args):
    """one leg, in a process of its own: prints one JSON line per scoring"""
    import torch
    from versalignlib_amd import build, hipkernel
    n = args.pairs
    reads, refs = _batch(n)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    for name, sc in _scorings():
        rec = {"leg": args.leg, "label": args.label, "scoring": name, "pairs": n}
        if args.leg == "sweep":
            eng = _SweepEngine(os.path.abspath(args.lib) if args.lib else build.HIP_PLUGIN, sc)
            scores = torch.empty(n, dtype=torch.int16, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            med, best = _timed(lambda: eng.score(d_reads, d_refs, scores, st), args.reps)
            rec["ran"] = "score_device, band %d" % BAND
            rec["checksum"] = int(scores.to(torch.int64).sum())
            eng.close()
            rec.update(ms_median=round(med, 3), ms_min=round(best, 3), us_per_pair=round(1e3 * med / n, 4))
            print("RESULT " + json.dumps(rec), flush=True)
            continue
        eng = hipkernel.Engine(R, F, sc)
        if args.leg == "placed":
            eng.set_band_width(BAND)
            eng.set_band_placed(1)
            placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
            med, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), args.reps)
            rec["ran"] = eng.describe(0, n)["ran_placed"]
            scores = eng.score_device(0, d_reads, d_refs)
            torch.cuda.synchronize()
            rec["score_equals_sweep"] = bool((placed[:, 0] == scores.to(torch.int32)).all())
            rec["checksum"] = int(placed[:, 0].to(torch.int64).sum())
            rec["ends_checksum"] = int(placed[:, 1:].to(torch.int64).sum())
        elif args.leg == "align":
            eng.set_band_width(BAND)
            eng.set_band_alignments(1)
            recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
            ops = torch.empty((n, 4096), dtype=torch.int32, device="cuda")
            med, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=4096, out=(recs, ops)), args.reps)
            rec["ran"] = eng.describe(0, n)["ran_align_fill"]
        else:
            placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
            med, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), args.reps)
            rec["ran"] = eng.describe(0, n)["ran_placed"]
        eng.close()
        rec.update(ms_median=round(med, 3), ms_min=round(best, 3), us_per_pair=round(1e3 * med / n, 4))
        print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--pairs", type=int, default=32768)
    ap.add_argument("--align-pairs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2, help="how often the sweep runs on each library")
    ap.add_argument("--leg", default="")
    ap.add_argument("--label", default="")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.leg:
        child(args)
        return
    legs = []
    for _ in range(args.rounds):
        if args.parent_lib:
            legs.append(("sweep", "parent", args.parent_lib, args.pairs))
        legs.append(("sweep", "this tree", "", args.pairs))
    legs += [("placed", "this tree", "", args.pairs), ("align", "this tree", "", args.align_pairs), ("strip", "this tree", "", args.align_pairs)]
    results = []
    for leg, label, lib, pairs in legs:
        cmd = [sys.executable, "-m", "tools.placed_band_bench", "--leg", leg, "--label", label, "--pairs", str(pairs), "--reps", str(args.reps)]
        if lib:
            cmd += ["--lib", lib]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=420)
        if proc.returncode != 0:
            print(proc.stdout[-3000:])
            raise SystemExit("leg %s (%s) failed with status %d: nothing more is started" % (leg, label, proc.returncode))
        for line in proc.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                results.append(r)
                print("%-7s %-10s %-7s %6d pairs %10.3f ms (min %10.3f)  %8.4f us / pair  %s" %
                      (r["leg"], r["label"], r["scoring"], r["pairs"], r["ms_median"], r["ms_min"], r["us_per_pair"], r["ran"]), flush=True)
    summary = {}
    for name in ("linear", "affine"):
        def med_of(leg, label):
            xs = [r["ms_median"] for r in results if r["leg"] == leg and r["label"] == label and r["scoring"] == name]
            return xs
        here, parent = med_of("sweep", "this tree"), med_of("sweep", "parent")
        placed = [r for r in results if r["leg"] == "placed" and r["scoring"] == name][0]
        per_pair = {leg: [r["us_per_pair"] for r in results if r["leg"] == leg and r["scoring"] == name][0] for leg in ("placed", "align", "strip")}
        summary[name] = {"sweep_ms_this_tree": here, "sweep_ms_parent": parent,
                         "sweep_checksums_equal": len({r["checksum"] for r in results if r["leg"] == "sweep" and r["scoring"] == name}) == 1,
                         "placed_ms": placed["ms_median"], "placed_over_sweep": round(placed["ms_median"] / statistics.median(here), 3),
                         "predicted_placed_over_sweep": list(PREDICTED[name]), "placed_score_equals_sweep": placed["score_equals_sweep"],
                         "us_per_pair": per_pair, "align_over_placed_per_pair": round(per_pair["align"] / per_pair["placed"], 2),
                         "strip_over_placed_per_pair": round(per_pair["strip"] / per_pair["placed"], 2)}
    print(json.dumps({"tool": "placed_band_bench", "shape": [R, F], "band": BAND, "summary": summary}))


if __name__ == "__main__":
    main()
