"""What placed scores on int32 cells (placed_wide = 1) cost, in one run, at the two shapes the key was built for:

  long ...... 10 kbp x 10 kbp, 4,096 pairs, match 5 / mismatch -4 / gaps -6 (affine: open -8, extend -2): out of int16 by the
              scoring (10,000 x 5 + 1 > 32,000), score_width = 0;
  short ..... 150 x 500, 1,048,576 pairs, match 2 / mismatch -1 / gaps -3 (affine: open -5, extend -1), at score_width = 32.

Per shape, linear and affine gaps:

  wide ...... score_placed_device under placed_wide = 1 ("ran_placed": "wide"), with the placed scratch the engine then holds;
  cigar ..... align_cigar_device on the same call -- what a caller paid for a score and an end cell before the key -- with the
              pointer scratch it holds ("align_scratch_bytes"), checked to give the same score and end cell;
  sweep32 ... score_device under score_width = 32: the int32 score sweep, the floor that end-cell tracking adds to;
  narrow .... the int16 placed routes on an in-range scoring of the same shape (match 2 / -1 / -3, affine -5 / -1; score_width
              0): what one pair per register costs -- on this tree's library and, with --parent-lib, on a library built from the
              parent commit, alternating, so that the file shows the run-to-run spread of one library beside the difference
              between the two (those routes are meant to be the same code);
  span ...... (long only) score_span_device under placed_wide = 1, beside two placed_wide calls.

  python -m tools.placed_wide_bench [--parent-lib PATH] [--reps 3] [--rounds 2] [--shapes long,short]

Every leg is a fresh child process (one engine family per process, nothing shared but the device), run one after the other
under a time limit of its own; the first that fails ends the run.  Inputs are resident on the device; every call is timed with
events around it on one stream after two warm-up calls; the median and the minimum of --reps launches are printed, then a JSON
summary with the wide / sweep32 ratio beside the ratio predicted from instruction counts (PREDICTED below; DESIGN.md has the
count).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

SHAPES = {
    # name: (R, F, pairs, score_width of the wide legs, (match, mismatch, gap), (open, extend))
    "long": (10000, 10000, 4096, 0, (5, -4, -6), (-8, -2)),
    "short": (150, 500, 1 << 20, 32, (2, -1, -3), (-5, -1)),
}
NARROW = ((2, -1, -3), (-5, -1))            # in range at both shapes
# Predicted wide / sweep32 ratio from instruction counts (tools/isa_histogram.py: --part placed, score_placed_wide_kernel<8, *>,
# against --part main, score_long_kernel<64, 8, SW, SYM, WIDE, *>; issue cycles per wave at 4.3 per half-rate and 2.6 per
# full-rate VALU instruction).  Both hot loops cover 16 cells per lane (the placed sweep: one step of two pairs; the score sweep:
# two steps of one pair).  The tool's loop of the placed sweep is 604 (linear) / 839 (affine) cycles, of which 121 / 137 belong
# to the ring refill and the boundary-row loads that run once per 64 steps: a step is 483 / 702 cycles against the score
# sweep's 279 / 633.
PREDICTED = {"linear": round(483 / 279, 2), "affine": round(702 / 633, 2)}


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


def _batch(R, F, n, seed=7, block=64):
    import numpy as np
    from versalignlib_amd import synth
    reads, refs = synth.make_pairs(block, R, F, seed=seed, sub_rate=0.1, indel_rate=0.01)
    reps = (n + block - 1) // block
    return np.tile(reads, (reps, 1))[:n].copy(), np.tile(refs, (reps, 1))[:n].copy()


def _scorings(lin, aff):
    from versalignlib_amd import hipkernel
    m, mm, g = lin
    return (("linear", hipkernel.Scoring.make(m, mm, g, g)), ("affine", hipkernel.Scoring.make(m, mm, g, g, aff[0], aff[1], aff[0], aff[1])))


class _PlacedEngine:
    """The entry points the narrow leg needs, bound by hand: the same calls on this tree's library and on one built from an
    earlier commit (which hipkernel.lib() rightly refuses to load: it lacks the newer symbols)"""

    def __init__(self, path, R, F, scoring):
        import ctypes
        self.L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        self.L.valign_hip_engine_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(vp)]
        self.L.valign_hip_engine_destroy.restype = None
        self.L.valign_hip_engine_destroy.argtypes = [vp]
        self.L.valign_hip_score_placed_device.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, vp, vp, vp, vp]
        self.L.valign_hip_describe.argtypes = [vp, ctypes.c_int, ctypes.c_longlong, ctypes.c_char_p, ctypes.c_int]
        self.L.valign_hip_last_error.restype = ctypes.c_char_p
        self.h = vp()
        self._check(self.L.valign_hip_engine_create(0, R, F, ctypes.addressof(scoring), 0, 0, ctypes.byref(self.h)))

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.valign_hip_last_error().decode(errors="replace"))

    def placed(self, d_reads, d_refs, out, stream):
        self._check(self.L.valign_hip_score_placed_device(self.h, 0, d_reads.shape[0], d_reads.data_ptr(), d_refs.data_ptr(), out.data_ptr(), stream))

    def describe(self, n):
        import ctypes
        buf = ctypes.create_string_buffer(8192)
        self._check(self.L.valign_hip_describe(self.h, 0, n, buf, 8192))
        return json.loads(buf.value.decode())

    def close(self):
        self.L.valign_hip_engine_destroy(self.h)


def child(args):
    """one leg, in a process of its own: prints one JSON line per scoring"""
    import torch
    from versalignlib_amd import build, hipkernel
    R, F, n, width, lin, aff = SHAPES[args.shape]
    reads, refs = _batch(R, F, n)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    del reads, refs
    narrow = args.leg == "narrow"
    for name, sc in _scorings(*(NARROW if narrow else (lin, aff))):
        rec = {"shape": args.shape, "leg": args.leg, "label": args.label, "scoring": name, "pairs": n}
        if narrow:
            eng = _PlacedEngine(os.path.abspath(args.lib) if args.lib else build.HIP_PLUGIN, R, F, sc)
            placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
            st = torch.cuda.current_stream().cuda_stream
            med, best = _timed(lambda: eng.placed(d_reads, d_refs, placed, st), args.reps)
            rec["ran"] = eng.describe(n)["ran_placed"]
            rec["checksum"] = int(placed.to(torch.int64).sum())
            eng.close()
        else:
            eng = hipkernel.Engine(R, F, sc)
            eng.set_score_width(width)
            if args.leg in ("wide", "span"):
                eng.set_placed_wide(1)
            if args.leg == "wide":
                placed = torch.empty((n, 3), dtype=torch.int32, device="cuda")
                med, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=placed), args.reps)
                d = eng.describe(0, n)
                rec.update(ran=d["ran_placed"], placed_scratch_bytes=d["placed_scratch_bytes"], checksum=int(placed.to(torch.int64).sum()),
                           score_max=int(placed[:, 0].max()))
            elif args.leg == "span":
                spans = torch.empty((n, 5), dtype=torch.int32, device="cuda")
                med, best = _timed(lambda: eng.score_span_device(0, d_reads, d_refs, out=spans), args.reps)
                d = eng.describe(0, n)
                rec.update(ran=d["ran_span"], span_ref_length=d["span_ref_length"], checksum=int(spans.to(torch.int64).sum()))
            elif args.leg == "cigar":
                recs = torch.empty((n, 6), dtype=torch.int32, device="cuda")
                ops = torch.empty((n, 8), dtype=torch.int32, device="cuda")
                med, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=8, out=(recs, ops)), args.reps)
                d = eng.describe(0, n)
                # valign_hip_aln: read_begin, read_end, ref_begin, ref_end, score, n_ops -> the placed record's three fields
                rec.update(ran=d["ran_align_fill"], align_scratch_bytes=d["align_scratch_bytes"], align_ptr_bytes_per_pair=d["align_ptr_bytes_per_pair"],
                           checksum=int(recs[:, [4, 1, 3]].to(torch.int64).sum()))
            else:           # sweep32
                scores = torch.empty(n, dtype=torch.int16, device="cuda")
                med, best = _timed(lambda: eng.score_device(0, d_reads, d_refs, scores=scores), args.reps)
                rec.update(ran="score_device, " + eng.describe(0, n)["ran_score_cells"], checksum=int(scores.to(torch.int64).sum()))
            eng.close()
        rec.update(ms_median=round(med, 3), ms_min=round(best, 3), us_per_pair=round(1e3 * med / n, 4))
        print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="how often the narrow leg runs on each library")
    ap.add_argument("--shapes", default="long,short")
    ap.add_argument("--leg", default="")
    ap.add_argument("--shape", default="long")
    ap.add_argument("--label", default="")
    ap.add_argument("--lib", default="")
    args = ap.parse_args()
    if args.leg:
        child(args)
        return
    results = []
    for shape in args.shapes.split(","):
        legs = [("wide", "this tree", ""), ("sweep32", "this tree", ""), ("cigar", "this tree", "")]
        for _ in range(args.rounds):
            if args.parent_lib:
                legs.append(("narrow", "parent", args.parent_lib))
            legs.append(("narrow", "this tree", ""))
        if shape == "long":
            legs.append(("span", "this tree", ""))
        for leg, label, lib in legs:
            cmd = [sys.executable, "-m", "tools.placed_wide_bench", "--leg", leg, "--shape", shape, "--label", label, "--reps", str(args.reps)]
            if lib:
                cmd += ["--lib", lib]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if proc.returncode != 0:
                print(proc.stdout[-3000:])
                raise SystemExit("leg %s / %s (%s) failed with status %d: nothing more is started" % (shape, leg, label, proc.returncode))
            for line in proc.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    results.append(r)
                    extra = "".join("  %s %.1f MB" % (k, r[k] / 1e6) for k in ("placed_scratch_bytes", "align_scratch_bytes") if k in r)
                    print("%-5s %-7s %-10s %-7s %8d pairs %10.3f ms (min %10.3f)  %9.4f us / pair  %s%s" %
                          (r["shape"], r["leg"], r["label"], r["scoring"], r["pairs"], r["ms_median"], r["ms_min"], r["us_per_pair"], r["ran"], extra), flush=True)
    summary = {}
    for shape in args.shapes.split(","):
        summary[shape] = {}
        for name in ("linear", "affine"):
            def of(leg, label="this tree"):
                return [r for r in results if r["shape"] == shape and r["leg"] == leg and r["label"] == label and r["scoring"] == name]
            wide, sweep, cigar = of("wide")[0], of("sweep32")[0], of("cigar")[0]
            here, parent = [r["ms_median"] for r in of("narrow")], [r["ms_median"] for r in of("narrow", "parent")]
            s = {"wide_ms": wide["ms_median"], "sweep32_ms": sweep["ms_median"], "cigar_ms": cigar["ms_median"], "cigar_ran": cigar["ran"],
                 "wide_over_sweep32": round(wide["ms_median"] / sweep["ms_median"], 3), "predicted_wide_over_sweep32": PREDICTED[name],
                 "cigar_over_wide": round(cigar["ms_median"] / wide["ms_median"], 2),
                 "wide_equals_cigar_records": wide["checksum"] == cigar["checksum"],
                 "placed_scratch_bytes": wide["placed_scratch_bytes"], "align_scratch_bytes": cigar["align_scratch_bytes"],
                 "narrow_ran": of("narrow")[0]["ran"], "narrow_ms_this_tree": here, "narrow_ms_parent": parent,
                 "narrow_checksums_equal": len({r["checksum"] for r in of("narrow") + of("narrow", "parent")}) == 1,
                 "wide_over_narrow": round(wide["ms_median"] / statistics.median(here), 3)}
            if of("span"):
                s.update(span_ms=of("span")[0]["ms_median"], span_ran=of("span")[0]["ran"], span_ref_length=of("span")[0]["span_ref_length"],
                         span_over_two_wide=round(of("span")[0]["ms_median"] / (2 * wide["ms_median"]), 3))
            summary[shape][name] = s
    print(json.dumps({"tool": "placed_wide_bench", "shapes": {k: list(v[:4]) for k, v in SHAPES.items() if k in summary}, "summary": summary}))


if __name__ == "__main__":
    main()
