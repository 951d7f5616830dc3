"""What banded extension alignments (extend_band_align = 1 under a band with extend_band = 1) cost against banded extension scores
on the same call, in one process: 10 kbp x 10 kbp, 4,096 pairs, match 5 / mismatch -4 / gaps -6 (affine: open -8, extend -2), linear
and affine gaps, band_width 1000 and 200, from the best cell (end_bonus -1) and from the read end (INT32_MAX).

The prediction, written before the first timed run (profiles/r30_extend_band_align.txt): the fill costs the banded score sweep x the
ratio of the two hot loops' modelled issue cycles (tools/isa_histogram.py --part extend_align --kernel
score_extend_wide_kernelILi8ELb0ELb1ELb1 / Lb1ELb1ELb1 against --part extend ...ELb1ELb0: 924 / 612 and 1503 / 850); the pointer
stream is far below what HBM takes in that time.

    python -m tools.extend_band_align_bench [--reps 3] [--rounds 2] [--pairs 4096] [--no-context]

Inputs are resident on the device; the legs of a scoring and band take turns, round after round; every call is timed with events
around it on one stream after two warm-up calls; per leg the median and the minimum over all rounds are printed; then, for context
only (another band definition: Smith-Waterman on the scaled diagonal), align_cigar_device under band_alignments at band_width 512;
then a JSON summary with the pointer bytes per pair, the scratch held and the chunk count.  The split into fill, walk and encoder
is a kernel trace's (rocprofv3 --kernel-trace --stats -- python -m tools.extend_band_align_bench --reps 1 --rounds 1)."""
import argparse
import json
import statistics

from tools.placed_wide_bench import _batch, _scorings, _timed

R, F = 10000, 10000
LIN, AFF = (5, -4, -6), (-8, -2)
BANDS = (1000, 200)
FILL = {"linear": 924 / 612, "affine": 1503 / 850}         # modelled issue cycles of one step, fill / banded score sweep
ALWAYS = 2 ** 31 - 1
STRIDE = 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--no-context", action="store_true")
    args = ap.parse_args()
    import torch
    from versalignlib_amd import hipkernel
    n = args.pairs
    reads, refs = _batch(R, F, n)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    del reads, refs
    out = (torch.empty((n, 6), dtype=torch.int32, device="cuda"), torch.empty((n, STRIDE), dtype=torch.int32, device="cuda"),
           torch.empty((n, 5), dtype=torch.int32, device="cuda"))
    scores = torch.empty((n, 5), dtype=torch.int32, device="cuda")
    summary = {}
    for name, sc in _scorings(LIN, AFF):
        for band in BANDS:
            eng = hipkernel.Engine(R, F, sc)
            eng.set_band_width(band)
            eng.set_extend_band(1)
            eng.set_extend_band_align(1)
            legs = {"scores": lambda: eng.score_extend_device(0, d_reads, d_refs, out=scores),
                    "best cell": lambda: eng.align_extend_device(0, d_reads, d_refs, end_bonus=-1, ops_stride=STRIDE, out=out),
                    "read end": lambda: eng.align_extend_device(0, d_reads, d_refs, end_bonus=ALWAYS, ops_stride=STRIDE, out=out)}
            times = {leg: ([], []) for leg in legs}
            for _ in range(args.rounds):
                for leg, fn in legs.items():
                    med, best = _timed(fn, args.reps)
                    times[leg][0].append(med)
                    times[leg][1].append(best)
            d = eng.describe(0, n)
            assert d["ran_extend_align"] == "band" and d["ran_extend"] == "band", d
            torch.cuda.synchronize()
            recs = out[0].to(torch.int64)
            assert bool((out[2] == scores).all()), "the extension records differ from the scores'"
            rec = {leg: {"ms_median": round(statistics.median(t[0]), 3), "ms_min": round(min(t[1]), 3), "round_medians": [round(m, 3) for m in t[0]]} for leg, t in times.items()}
            base = rec["scores"]["ms_median"]
            rec.update(ptr_bytes_per_pair=d["align_ptr_bytes_per_pair"], chunks=d["ran_extend_align_chunks"], pointer_scratch_bytes=d["extend_align_scratch_bytes"],
                       strip_scratch_bytes=d["placed_scratch_bytes"], rows_scratch_bytes=d["cigar_rows_scratch_bytes"], predicted_fill_over_scores=round(FILL[name], 3),
                       aligned=int((recs[:, 5] > 0).sum()), ops_max=int(recs[:, 5].max()), read_end_reached=int((recs[:, 1] == R).sum()))
            for leg in ("best cell", "read end"):
                rec[leg]["over_scores"] = round(rec[leg]["ms_median"] / base, 3)
            print("%-7s band %-5d scores %9.3f ms | alignments from the best cell %9.3f ms (x %.2f), from the read end %9.3f ms (x %.2f) | predicted fill / scores %.2f | "
                  "%d pointer bytes per pair, %d chunk(s), scratch: pointers %.1f GB, rows %.2f GB, strips %.2f GB | %d of %d aligned (read-end leg), at most %d ops"
                  % (name, band, base, rec["best cell"]["ms_median"], rec["best cell"]["over_scores"], rec["read end"]["ms_median"], rec["read end"]["over_scores"], FILL[name],
                     rec["ptr_bytes_per_pair"], rec["chunks"], rec["pointer_scratch_bytes"] / 1e9, rec["rows_scratch_bytes"] / 1e9, rec["strip_scratch_bytes"] / 1e9,
                     rec["aligned"], n, rec["ops_max"]), flush=True)
            summary["%s %d" % (name, band)] = rec
            eng.close()
        if not args.no_context:          # another band definition, for context only
            eng = hipkernel.Engine(R, F, sc)
            eng.set_band_width(512)
            eng.set_band_alignments(1)
            med, best = _timed(lambda: eng.align_cigar_device(0, d_reads, d_refs, ops_stride=STRIDE, out=(out[0], out[1])), args.reps)
            d = eng.describe(0, n)
            summary["%s context" % name] = {"ms_median": round(med, 3), "ms_min": round(best, 3), "ran_align_fill": d["ran_align_fill"], "ptr_bytes_per_pair": d["align_ptr_bytes_per_pair"]}
            print("%-7s context: align_cigar_device under band_alignments, band_width 512 (%s): %9.3f ms (min %9.3f), %d pointer bytes per pair"
                  % (name, d["ran_align_fill"], med, best, d["align_ptr_bytes_per_pair"]), flush=True)
            eng.close()
    print(json.dumps({"tool": "extend_band_align_bench", "shape": [R, F, n], "summary": summary}))


if __name__ == "__main__":
    main()
