"""What banded extension scores (extend_band = 1 under a band) cost against the unbanded int32 extension sweep (extend_wide = 1),
in one process, at the shape extend_wide was built for: 10 kbp x 10 kbp, 4,096 pairs, match 5 / mismatch -4 / gaps -6 (affine:
open -8, extend -2), linear and affine gaps, band_width 1000 and 200.

The prediction, written before the first timed run (profiles/r28_extend_band.txt): the banded time is the unbanded time of the same
process x window steps / unbanded steps (the step counts of extend_band_strip, restated below from extend_band_plan.h) x the ratio
of the two hot loops' modelled issue cycles (tools/isa_histogram.py --part extend --kernel score_extend_wide_kernelILi8ELb0ELb1 /
Lb1ELb1 against ...ELb0ELb0 / Lb1ELb0: 612 / 602 and 850 / 822).

    python -m tools.extend_band_bench [--reps 5] [--rounds 3] [--pairs 4096]

Inputs are resident on the device; the three engines of a scoring (unbanded, band 1000, band 200) take turns, round after round;
every call is timed with events around it on one stream after two warm-up calls; per leg the median and the minimum over all
rounds are printed, and the spread of the rounds' medians; then a JSON summary.
"""
import argparse
import json
import statistics

from tools.placed_wide_bench import _batch, _scorings, _timed

R, F = 10000, 10000
LIN, AFF = (5, -4, -6), (-8, -2)
BANDS = (1000, 200)
MASK = {"linear": 612 / 602, "affine": 850 / 822}         # modelled issue cycles of one step, banded / unbanded


def window_steps(strip, cols, w):
    """steps of one 512-row strip's window: extend_band_strip's t_end - t_begin (0: empty)"""
    row0 = strip * 512
    first, end = max(row0 - w, 0), min(row0 + 511 + w + 1, cols)
    return 0 if first >= end else end + 63 - first // 64 * 64


def step_ratio(band_width):
    strips = (R + 511) // 512
    return sum(window_steps(s, F, band_width // 2) for s in range(strips)) / (strips * (F + 63))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4096)
    args = ap.parse_args()
    import torch
    from versalignlib_amd import hipkernel
    n = args.pairs
    reads, refs = _batch(R, F, n)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    del reads, refs
    summary = {}
    for name, sc in _scorings(LIN, AFF):
        legs = {}
        for band in (0,) + BANDS:
            eng = hipkernel.Engine(R, F, sc)
            if band:
                eng.set_band_width(band)
                eng.set_extend_band(1)
            else:
                eng.set_extend_wide(1)
            legs[band] = {"eng": eng, "out": torch.empty((n, 5), dtype=torch.int32, device="cuda"), "medians": [], "mins": []}
        for _ in range(args.rounds):
            for band, leg in legs.items():
                med, best = _timed(lambda: leg["eng"].score_extend_device(0, d_reads, d_refs, out=leg["out"]), args.reps)
                leg["medians"].append(med)
                leg["mins"].append(best)
        rec = {}
        for band, leg in legs.items():
            d = leg["eng"].describe(0, n)
            assert d["ran_extend"] == ("band" if band else "wide"), d["ran_extend"]
            out = leg["out"].to(torch.int64)
            rec[band] = {"ms_median": round(statistics.median(leg["medians"]), 3), "ms_min": round(min(leg["mins"]), 3),
                         "round_medians": [round(m, 3) for m in leg["medians"]], "ran": d["ran_extend"],
                         "score_max": int(out[:, 0].max()), "unreached": int((out[:, 3] == hipkernel.EXTEND_UNREACHED).sum()),
                         "same_score_as_unbanded": int((out[:, 0] == legs[0]["out"][:, 0].to(torch.int64)).sum()),
                         "scratch_bytes": d["placed_scratch_bytes"]}
            leg["eng"].close()
        free = rec[0]["ms_median"]
        print("%-7s unbanded   %9.3f ms (min %9.3f)  rounds %s" % (name, free, rec[0]["ms_min"], rec[0]["round_medians"]), flush=True)
        for band in BANDS:
            r = rec[band]
            r["step_ratio"] = round(step_ratio(band), 4)
            r["predicted_ms"] = round(free * step_ratio(band) * MASK[name], 3)
            r["measured_over_predicted"] = round(r["ms_median"] / r["predicted_ms"], 3)
            r["speedup"] = round(free / r["ms_median"], 2)
            print("%-7s band %-5d %9.3f ms (min %9.3f)  rounds %s  predicted %8.3f ms (steps x %.4f, mask x %.3f)  measured / predicted %.3f  %.2f x faster; "
                  "%d of %d pairs keep the unbanded score, %d unreached" % (name, band, r["ms_median"], r["ms_min"], r["round_medians"], r["predicted_ms"], r["step_ratio"],
                                                                             MASK[name], r["measured_over_predicted"], r["speedup"], r["same_score_as_unbanded"], n, r["unreached"]), flush=True)
        summary[name] = {str(k): v for k, v in rec.items()}
    print(json.dumps({"tool": "extend_band_bench", "shape": [R, F, n], "summary": summary}))


if __name__ == "__main__":
    main()
