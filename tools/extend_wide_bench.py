"""What extension scores on int32 cells and row strips (extend_wide = 1) cost, in one run, at the two shapes the key was built for:

  long ...... 10 kbp x 10 kbp, 4,096 pairs, match 5 / mismatch -4 / gaps -6 (affine: open -8, extend -2): refused without the key
              by the read's length (and by the scoring: 10,000 x 5 > 32,000), score_width = 0;
  short ..... 150 x 500, 1,048,576 pairs, match 2 / mismatch -1 / gaps -3 (affine: open -5, extend -1), at score_width = 32.

Per shape, linear and affine gaps:

  extend .... score_extend_device under extend_wide = 1 ("ran_extend": "wide"), with the strip scratch the engine then holds;
  placed .... (long) score_placed_device under placed_wide = 1 on the same call: the int32 placed sweep the kernel was derived from
              -- the prediction is this leg's time x the ratio of the two hot loops' VALU counts (PREDICTED below);
  rows ...... (short) score_extend_device with the key off and score_width = 0: the packed int16 register sweep, checked to give
              the same records.

  python -m tools.extend_wide_bench [--reps 3] [--shapes long,short]

Every leg is a fresh child process, run one after the other under a time limit of its own; the first that fails ends the run.
Inputs are resident on the device; every call is timed with events around it on one stream after two warm-up calls; the median
and the minimum of --reps launches are printed, then a JSON summary.
"""
import argparse
import json
import subprocess
import sys

from tools.placed_wide_bench import _batch, _scorings, _timed

SHAPES = {
    # name: (R, F, pairs, score_width of the wide leg, (match, mismatch, gap), (open, extend))
    "long": (10000, 10000, 4096, 0, (5, -4, -6), (-8, -2)),
    "short": (150, 500, 1 << 20, 32, (2, -1, -3), (-5, -1)),
}
# Predicted extend / placed ratio: VALU instructions of one trip of the two hot loops (tools/isa_histogram.py --part extend
# --kernel score_extend_wide_kernelILi8ELb0 / Lb1 against --part placed --kernel score_placed_wide_kernelILi8ELb0 / Lb1): 202 / 203
# and 286 / 292 -- the signed adds stand where the saturating subtracts stood, the column mask of the row tracking costs scalar
# instructions (89 / 108 against 68 / 79), which the count does not see.
PREDICTED = {"linear": round(202 / 203, 3), "affine": round(286 / 292, 3)}


def child(args):
    """one leg, in a process of its own: prints one JSON line per scoring"""
    import torch
    from versalignlib_amd import hipkernel
    R, F, n, width, lin, aff = SHAPES[args.shape]
    reads, refs = _batch(R, F, n)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    del reads, refs
    for name, sc in _scorings(lin, aff):
        rec = {"shape": args.shape, "leg": args.leg, "scoring": name, "pairs": n}
        eng = hipkernel.Engine(R, F, sc)
        if args.leg == "placed":
            eng.set_placed_wide(1)
            eng.set_score_width(width)
            out = torch.empty((n, 3), dtype=torch.int32, device="cuda")
            med, best = _timed(lambda: eng.score_placed_device(0, d_reads, d_refs, out=out), args.reps)
            d = eng.describe(0, n)
            rec.update(ran=d["ran_placed"], scratch_bytes=d["placed_scratch_bytes"], checksum=int(out[:, 0].to(torch.int64).sum()))
        else:
            wide = args.leg == "extend"
            eng.set_extend_wide(1 if wide else 0)
            eng.set_score_width(width if wide else 0)
            out = torch.empty((n, 5), dtype=torch.int32, device="cuda")
            med, best = _timed(lambda: eng.score_extend_device(0, d_reads, d_refs, out=out), args.reps)
            d = eng.describe(0, n)
            rec.update(ran=d["ran_extend"], scratch_bytes=d["placed_scratch_bytes"], checksum=int(out.to(torch.int64).sum()), score_max=int(out[:, 0].max()))
        eng.close()
        rec.update(ms_median=round(med, 3), ms_min=round(best, 3), us_per_pair=round(1e3 * med / n, 4))
        print("RESULT " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default="long,short")
    ap.add_argument("--leg", default="")
    ap.add_argument("--shape", default="long")
    args = ap.parse_args()
    if args.leg:
        child(args)
        return
    results = []
    for shape in args.shapes.split(","):
        for leg in ("extend", "placed" if shape == "long" else "rows"):
            cmd = [sys.executable, "-m", "tools.extend_wide_bench", "--leg", leg, "--shape", shape, "--reps", str(args.reps)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
            if proc.returncode != 0:
                print(proc.stdout[-3000:])
                raise SystemExit("leg %s / %s failed with status %d: nothing more is started" % (shape, leg, proc.returncode))
            for line in proc.stdout.splitlines():
                if line.startswith("RESULT "):
                    r = json.loads(line[7:])
                    results.append(r)
                    print("%-5s %-7s %-7s %8d pairs %10.3f ms (min %10.3f)  %9.4f us / pair  %-5s scratch %.1f MB" %
                          (r["shape"], r["leg"], r["scoring"], r["pairs"], r["ms_median"], r["ms_min"], r["us_per_pair"], r["ran"], r["scratch_bytes"] / 1e6), flush=True)
    summary = {}
    for shape in args.shapes.split(","):
        summary[shape] = {}
        for name in ("linear", "affine"):
            def of(leg):
                return [r for r in results if r["shape"] == shape and r["leg"] == leg and r["scoring"] == name][0]
            ext = of("extend")
            s = {"extend_wide_ms": ext["ms_median"], "scratch_bytes": ext["scratch_bytes"], "score_max": ext["score_max"]}
            if shape == "long":
                placed = of("placed")
                s.update(placed_wide_ms=placed["ms_median"], extend_over_placed=round(ext["ms_median"] / placed["ms_median"], 3),
                         predicted_extend_over_placed=PREDICTED[name], predicted_ms=round(placed["ms_median"] * PREDICTED[name], 1))
            else:
                rows = of("rows")
                s.update(rows_ms=rows["ms_median"], rows_ran=rows["ran"], wide_over_rows=round(ext["ms_median"] / rows["ms_median"], 2),
                         wide_equals_rows_records=ext["checksum"] == rows["checksum"])
            summary[shape][name] = s
    print(json.dumps({"tool": "extend_wide_bench", "shapes": {k: list(v[:4]) for k, v in SHAPES.items() if k in summary}, "summary": summary}))


if __name__ == "__main__":
    main()
