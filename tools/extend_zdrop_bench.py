"""What the extend_zdrop key costs where nothing drops, and what it saves where pairs drop, in one process, at the shape the int32
extension sweep was built for: 10 kbp x 10 kbp, 4,096 pairs, match 5 / mismatch -4 / gaps -6 (affine: open -8, extend -2), linear
and affine gaps, unbanded (extend_wide = 1) and under band_width 1000 (extend_band = 1); with --align the banded extension
alignments too (extend_band_align = 1, end_bonus -1).

    python -m tools.extend_zdrop_bench [--reps 5] [--rounds 3] [--pairs 4096] [--align] [--short]

Two sets of inputs, resident on the device: reads with 10 % substitutions and 1 % indels (nothing drops: Z = 2^29 against Z = 0),
and the same pairs with the read all A from row 2,000 on and the reference all C from column 2,000 on (the homology ends there: Z
= 400 against Z = 0; a RANDOM tail does not end it under these scores -- with gaps at -6 beside matches at 5 the best score of random
against random keeps growing, and nothing drops).  The engines of a
scoring and band take turns, round after round; every call is timed with events around it on one stream after two warm-up calls;
per leg the median and the minimum over all rounds are printed, then a JSON summary.  The prediction (profiles/
r31_extend_zdrop.txt) for the dropping legs is the Z = 0 time of the same inputs x the share of the sweep's steps in the strips that
run, which the tool prints from the count of skipped waves.  --short: 150 x 500, 65,536 pairs, unbanded under Z = 400 against the
register sweep without the key.  --rows: the same shape and pairs under the key extend_zdrop_rows -- the register sweep with both
keys off (the baseline), Z = 2^29 and Z = 400 on the register sweep's ZDROP instances, the same two on today's "wide" route (the key
off), and baseline, Z = 2^29 and Z = 400 for align_extend_device (end_bonus -1); Z = 400 runs on pairs whose homology ends at row 40
(A against C from there: the drop falls near row 140).  The legs of a scoring take turns, round after round."""
import argparse
import json
import statistics

from tools.extend_band_bench import window_steps
from tools.placed_wide_bench import _batch, _scorings, _timed

R, F = 10000, 10000
LIN, AFF = (5, -4, -6), (-8, -2)
BAND = 1000
END = 2000                      # the homology of the dropping inputs ends here
NEVER = 1 << 29


def steps_share(strips_run, band_width, rows=R, cols=F):
    """the share of the sweep's steps that lie in its first `strips_run` strips"""
    strips = (rows + 511) // 512
    per = [window_steps(s, cols, band_width // 2) if band_width else cols + 63 for s in range(strips)]
    return sum(per[:strips_run]) / sum(per)


def _engine(hipkernel, rows, cols, sc, band, Z, align):
    eng = hipkernel.Engine(rows, cols, sc)
    if band:
        eng.set_band_width(band)
        eng.set_extend_band(1)
        eng.set_extend_band_align(1 if align else 0)
    else:
        eng.set_extend_wide(1)
    eng.set_extend_zdrop(Z)
    return eng


def rows_legs(args, torch, hipkernel):
    rows, cols, n, end = 150, 500, 65536, 40
    reads, refs = _batch(rows, cols, n)
    cut, cut_refs = reads.copy(), refs.copy()
    cut[:, end:] = ord("A")
    cut_refs[:, end:] = ord("C")
    inputs = {"whole": (torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()), "ends": (torch.from_numpy(cut).cuda(), torch.from_numpy(cut_refs).cuda())}
    summary = {}
    for name, sc in _scorings(LIN, AFF):
        legs = {}
        #            inputs   Z      extend_zdrop_rows  alignments
        for leg_key in (("whole", 0, 0, False), ("whole", NEVER, 1, False), ("ends", 0, 0, False), ("ends", 400, 1, False), ("whole", NEVER, 0, False), ("ends", 400, 0, False),
                        ("whole", 0, 0, True), ("whole", NEVER, 1, True), ("ends", 0, 0, True), ("ends", 400, 1, True)):
            what, Z, key, align = leg_key
            eng = hipkernel.Engine(rows, cols, sc)
            eng.set_extend_zdrop(Z)
            eng.set_extend_zdrop_rows(key)
            rd, rf = inputs[what]
            leg = {"eng": eng, "medians": [], "mins": []}
            if align:
                leg["out"] = eng.align_extend_device(0, rd, rf, end_bonus=-1, ops_stride=64)
                leg["call"] = lambda e=eng, a=rd, b=rf, o=leg["out"]: e.align_extend_device(0, a, b, end_bonus=-1, ops_stride=64, out=o)
            else:
                leg["out"] = torch.empty((n, 5), dtype=torch.int32, device="cuda")
                leg["call"] = lambda e=eng, a=rd, b=rf, o=leg["out"]: e.score_extend_device(0, a, b, out=o)
            legs[leg_key] = leg
        for _ in range(args.rounds):
            for leg in legs.values():
                med, best = _timed(leg["call"], args.reps)
                leg["medians"].append(med)
                leg["mins"].append(best)
        rec = {}
        for (what, Z, key, align), leg in legs.items():
            d = leg["eng"].describe(0, n)
            ext = (leg["out"][2] if align else leg["out"]).to(torch.int64)
            rec[what, Z, key, align] = {"ms_median": round(statistics.median(leg["medians"]), 4), "ms_min": round(min(leg["mins"]), 4),
                                        "round_medians": [round(m, 4) for m in leg["medians"]], "ran": d["ran_extend_align" if align else "ran_extend"],
                                        "geometry": d["ran_extend_align_geometry" if align else "ran_extend_geometry"],
                                        "dropped": int((ext[:, 3] == hipkernel.EXTEND_UNREACHED).sum()), "read_end_median": int(ext[:, 1].median())}
            leg["eng"].close()
        for align in (False, True):
            for what, Z in (("whole", NEVER), ("ends", 400)):
                base, on = rec[what, 0, 0, align], rec[what, Z, 1, align]
                line = "%-7s 150 x 500 %-10s %-5s Z = 0 %8.4f ms (min %8.4f, %s %s) | Z = %-9d rows %8.4f ms (min %8.4f, %s) x %.4f, %d dropped, read_end median %d" % (
                    name, "alignments" if align else "scores", what, base["ms_median"], base["ms_min"], base["ran"], base["geometry"], Z, on["ms_median"], on["ms_min"], on["ran"],
                    on["ms_median"] / base["ms_median"], on["dropped"], on["read_end_median"])
                if not align:
                    wide = rec[what, Z, 0, False]
                    line += " | key off %8.4f ms (min %8.4f, %s): rows %.2f x faster" % (wide["ms_median"], wide["ms_min"], wide["ran"], wide["ms_median"] / on["ms_median"])
                print(line, flush=True)
        summary[name] = {"%s/%d/%d/%s" % (k[0], k[1], k[2], "align" if k[3] else "scores"): v for k, v in rec.items()}
    print(json.dumps({"tool": "extend_zdrop_bench", "mode": "rows", "shape": [rows, cols, n], "summary": summary}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--align", action="store_true", help="banded extension alignments in the place of the scores")
    ap.add_argument("--short", action="store_true", help="150 x 500 under the key against the register sweep without it")
    ap.add_argument("--rows", action="store_true", help="150 x 500 under extend_zdrop_rows: scores and alignments against the register sweep without the keys and against the wide route")
    args = ap.parse_args()
    import torch
    from versalignlib_amd import hipkernel
    if args.rows:
        return rows_legs(args, torch, hipkernel)
    if args.short:
        rows, cols, n = 150, 500, 65536
        reads, refs = _batch(rows, cols, n)
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        for name, sc in _scorings(LIN, AFF):
            out = {}
            for Z in (0, 400):
                eng = hipkernel.Engine(rows, cols, sc)
                eng.set_extend_zdrop(Z)
                buf = torch.empty((n, 5), dtype=torch.int32, device="cuda")
                med, best = _timed(lambda: eng.score_extend_device(0, d_reads, d_refs, out=buf), args.reps)
                out[Z] = (med, best, eng.describe(0, n)["ran_extend"])
                eng.close()
            print("%-7s 150 x 500, %d pairs: Z = 0 %8.3f ms (%s), Z = 400 %8.3f ms (%s): %.1f x slower" %
                  (name, n, out[0][0], out[0][2], out[400][0], out[400][2], out[400][0] / out[0][0]), flush=True)
        return
    n = args.pairs
    reads, refs = _batch(R, F, n)
    cut, cut_refs = reads.copy(), refs.copy()
    cut[:, END:] = ord("A")
    cut_refs[:, END:] = ord("C")
    inputs = {"whole": (torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()), "ends": (torch.from_numpy(cut).cuda(), torch.from_numpy(cut_refs).cuda())}
    del reads, cut, refs, cut_refs
    summary = {}
    for name, sc in _scorings(LIN, AFF):
        for band in ((BAND,) if args.align else (0, BAND)):
            legs = {}
            for what, Z in (("whole", 0), ("whole", NEVER), ("ends", 0), ("ends", 400)):
                eng = _engine(hipkernel, R, F, sc, band, Z, args.align)
                leg = {"eng": eng, "medians": [], "mins": []}
                rd, rf = inputs[what]
                if args.align:
                    leg["out"] = eng.align_extend_device(0, rd, rf, end_bonus=-1, ops_stride=64)
                    leg["call"] = lambda e=eng, a=rd, b=rf, o=leg["out"]: e.align_extend_device(0, a, b, end_bonus=-1, ops_stride=64, out=o)
                else:
                    leg["out"] = torch.empty((n, 5), dtype=torch.int32, device="cuda")
                    leg["call"] = lambda e=eng, a=rd, b=rf, o=leg["out"]: e.score_extend_device(0, a, b, out=o)
                legs[what, Z] = leg
            for _ in range(args.rounds):
                for leg in legs.values():
                    med, best = _timed(leg["call"], args.reps)
                    leg["medians"].append(med)
                    leg["mins"].append(best)
            rec = {}
            for (what, Z), leg in legs.items():
                d = leg["eng"].describe(0, n)
                ext = (leg["out"][2] if args.align else leg["out"]).to(torch.int64)
                rec[what, Z] = {"ms_median": round(statistics.median(leg["medians"]), 3), "ms_min": round(min(leg["mins"]), 3),
                                "round_medians": [round(m, 3) for m in leg["medians"]], "ran": d["ran_extend_align" if args.align else "ran_extend"],
                                "skipped_waves": d["extend_zdrop_skipped_waves"], "dropped": int((ext[:, 3] == hipkernel.EXTEND_UNREACHED).sum()),
                                "read_end_median": int(ext[:, 1].median())}
                leg["eng"].close()
            base, never, ends0, ends = rec["whole", 0], rec["whole", NEVER], rec["ends", 0], rec["ends", 400]
            strips = (R + 511) // 512
            run = strips - ends["skipped_waves"] / ((n + 1) // 2)
            share = steps_share(int(round(run)), band)
            tag = "%-7s %s%s" % (name, "band %d" % band if band else "unbanded", " alignments" if args.align else "")
            print("%s  Z = 0 %9.3f ms (min %9.3f) %s | Z = 2^29 %9.3f ms (min %9.3f) %s: x %.4f, %d dropped" %
                  (tag, base["ms_median"], base["ms_min"], base["round_medians"], never["ms_median"], never["ms_min"], never["round_medians"],
                   never["ms_median"] / base["ms_median"], never["dropped"]), flush=True)
            print("%s  homology ends at row %d: Z = 0 %9.3f ms (min %9.3f) | Z = 400 %9.3f ms (min %9.3f) %s: %.2f x faster; %d of %d pairs dropped, read_end median %d, "
                  "%.2f of %d strips run per wave, steps share %.4f -> predicted %.3f ms, measured / predicted %.3f" %
                  (tag, END, ends0["ms_median"], ends0["ms_min"], ends["ms_median"], ends["ms_min"], ends["round_medians"], ends0["ms_median"] / ends["ms_median"],
                   ends["dropped"], n, ends["read_end_median"], run, strips, share, ends0["ms_median"] * share, ends["ms_median"] / (ends0["ms_median"] * share)), flush=True)
            summary["%s/%d" % (name, band)] = {"%s/%d" % k: v for k, v in rec.items()}
    print(json.dumps({"tool": "extend_zdrop_bench", "shape": [R, F, n], "align": args.align, "summary": summary}))


if __name__ == "__main__":
    main()
