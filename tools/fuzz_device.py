#!/usr/bin/env python3
"""Randomised sweep of the flat device / host API (developer tool; run on the GPU box): hipkernel.Engine objects created and
destroyed by the hundred, score_device / align_device on torch tensors and random streams, score_host / align_host on numpy
arrays (with and without a registered destination), length-sorted batching, bands, pointer-scratch caps -- every result
against oracle/cpu_ref; placed Smith-Waterman scores (score_placed_device / _host) against tests/placed_ref.py and, under a band with
band_placed = 1, against tests/placed_band_ref.py; spanned scores (score_span_device / _host) against tests/span_ref.py wherever the
unbanded placed scores run, and refused under every band; suboptimal scores (score_subopt_device / _host, a random mask) against
tests/subopt_ref.py wherever placed scores ran on the register sweep -- and `--kind subopt` draws nothing but cases for them: shapes up
to 160 x 300 with a second, mutated copy of the read planted in the reference; `--kind span_cigar` draws nothing but cases for the
spanned CIGARs (align_span_device / _host against tests/span_cigar_ref.py: random shapes up to 320 x 900 and one in eight on the row
strips, scorings, extended, ops_stride, trace_checkpoints, pointer_scratch_cap_mb, placed_wide); `--kind extend` draws nothing but
cases for the extension scores (a third of them extend_wide = 1 cases -- long reads, scorings out of int16, score_width = 32; score_extend_device / _host against tests/extend_ref.py: random shapes up to 200 x 300, the four gap
forms at several scales, the engine's own or a forced geometry, planted extensions, ragged tails and interior junk); `--kind extend_band` draws nothing but cases for the banded extension scores
(extend_band = 1 under a band, against tests/extend_band_ref.py: random shapes of one to four 512-row strips, random bands from
w = 0 to the unbanded limit, the four gap forms, score_width 0 / 32, extend_wide 0 / 1, ragged tails); `--kind extend_zdrop` draws
the same cases with a random Z of extend_zdrop, a third of them without the band (against tests/extend_zdrop_ref.py: records and
the count of skipped waves); `--kind extend_zdrop_rows` draws the register-sweep cases of `--kind extend` under extend_zdrop_rows = 1
with a random Z, as scores or as alignments (against tests/extend_zdrop_ref.py with band_width = 0, and tests/extend_align_ref.py on
the reads cut at the drop rows); `--kind extend_band_align`
draws the same shapes and bands for banded extension alignments (extend_band_align = 1: align_extend_device / _host against
tests/extend_band_align_ref.py, from the best cell, from the read end and at bonus 20, extended, ops_stride, pointer_scratch_cap_mb);
`--kind extend_align`
draws nothing but cases for the extension alignments (align_extend_device / _host against tests/extend_align_ref.py: the register-sweep
cases of `--kind extend` with an end bonus, extended, ops_stride, with or without the extension records, pointer_scratch_cap_mb).  What tools/fuzz_parity.py does for the plugin ABI, for the entry points the tests of the device path
use; a process that runs it for minutes also exercises the library's set-up and tear-down far more often than the suite.

    python -X faulthandler tools/fuzz_device.py --seconds 300 --seed 1
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))     # band_nw_ref: the restated banded NW variant

import torch                                                       # noqa: E402

from oracle import cpu_ref                                          # noqa: E402
from versalignlib_amd import hipkernel, synth                      # noqa: E402
import band_nw_ref                                                 # noqa: E402
import extend_align_ref                                            # noqa: E402
import extend_band_ref                                             # noqa: E402
import extend_band_align_ref                                       # noqa: E402
import extend_ref                                                  # noqa: E402
import extend_zdrop_ref                                            # noqa: E402
import placed_band_ref                                             # noqa: E402
import placed_ref                                                  # noqa: E402
import span_cigar_ref                                              # noqa: E402
import span_ref                                                    # noqa: E402
import subopt_ref                                                  # noqa: E402


NW_BAND_CASES = [0]             # cases that also ran the NW variant under the band
PLACED_CASES = [0]              # cases that also ran placed Smith-Waterman scores
SPAN_CASES = [0]                # ... and spanned scores
SUBOPT_CASES = [0]              # ... and suboptimal scores
BAND_PLACED_CASES = [0]         # banded cases that also ran placed scores on the chain (band_placed = 1)


def draw(rng, kind=None):
    kind = kind or rng.choice(["short", "short", "mid", "long", "longref", "tiny"])
    if kind == "subopt":
        R, F = int(rng.integers(8, 161)), int(rng.integers(8, 301))
    elif kind == "tiny":
        R, F = int(rng.integers(1, 24)), int(rng.integers(1, 40))
    elif kind == "short":
        R, F = int(rng.integers(8, 400)), int(rng.integers(8, 900))
    elif kind == "mid":
        R, F = int(rng.integers(400, 2100)), int(rng.integers(200, 3000))
    elif kind == "longref":
        R, F = int(rng.integers(20, 400)), int(rng.integers(3000, 12000))
    else:
        R, F = int(rng.integers(2049, 5000)), int(rng.integers(50, 4000))
    n = int(max(1, min(rng.integers(1, 600), 5_000_000 // max(R * F, 1))))
    affine = bool(rng.random() < 0.45)
    match, mismatch = int(rng.integers(1, 6)), -int(rng.integers(0, 7))
    gr = -int(rng.integers(1, 9))
    gf = gr if rng.random() < 0.5 else -int(rng.integers(1, 9))
    aff = {}
    if affine:
        er, ef = -int(rng.integers(1, 4)), -int(rng.integers(1, 4))
        orr, of = er - int(rng.integers(0, 8)), ef - int(rng.integers(0, 8))
        if rng.random() < 0.6:
            of, ef = orr, er
        aff = dict(open_read=orr, ext_read=er, open_ref=of, ext_ref=ef)
    if kind == "subopt":            # nothing but the register sweep: no band, default tie-breaks
        return dict(R=R, F=F, n=n, affine=affine, match=match, mismatch=mismatch, gr=gr, gf=gf, aff=aff, seed=int(rng.integers(1, 1 << 30)), ragged=0,
                    band=0, stream=bool(rng.random() < 0.5), policy=0, cap_mb=0, host=bool(rng.random() < 0.3), threads=int(rng.integers(1, 9)), ckpt=False,
                    subopt_only=True)
    return dict(R=R, F=F, n=n, affine=affine, match=match, mismatch=mismatch, gr=gr, gf=gf, aff=aff,
                seed=int(rng.integers(1, 1 << 30)), ragged=int(rng.integers(0, 3)) if rng.random() < 0.3 else 0,
                band=int(rng.integers(8, 300)) * 2 if (rng.random() < 0.12 and R >= 64) else 0,
                stream=bool(rng.random() < 0.5), policy=1 if (not affine and rng.random() < 0.2) else 0,
                cap_mb=int(rng.integers(1, 64)) if rng.random() < 0.15 else 0, host=bool(rng.random() < 0.3),
                threads=int(rng.integers(1, 9)), ckpt=bool(kind == "long" and rng.random() < 0.5))     # long reads: checkpointed traceback


def run(c):
    R, F, n = c["R"], c["F"], c["n"]
    reads, refs = synth.make_pairs(n, R, F, seed=c["seed"], sub_rate=0.1, indel_rate=0.02 if n * R < 300_000 else 0.0, n_run_frac=0.1,
                                   short_frac=0.3, lowercase_frac=0.05, junk_frac=0.05)
    if c.get("subopt_only") and F > 16:
        # a second copy of the read's head, three bases changed, somewhere in the reference: a runner-up worth finding
        rng = np.random.default_rng(c["seed"])
        L = min(R, F // 2)
        for p in range(0, n, 2):
            copy = reads[p, :L].copy()
            copy[rng.integers(0, L, 3)] = ord("A")
            at = int(rng.integers(0, F - L + 1))
            refs[p, at:at + L] = copy
    osc = cpu_ref.Scoring.make(c["match"], c["mismatch"], c["gr"], c["gf"], *(c["aff"].values() if c["affine"] else ()))
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(c["match"], c["mismatch"], c["gr"], c["gf"], **c["aff"]))
    try:
        if c["ragged"]:
            eng.set_ragged_batching(c["ragged"])
        if c["policy"]:
            eng.set_traceback_policy(1)
        if c["cap_mb"]:
            eng.set_pointer_scratch_cap_mb(c["cap_mb"])
        if c.get("ckpt"):
            eng.set_trace_checkpoints(1)
        stream = torch.cuda.Stream() if c["stream"] else None
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        torch.cuda.synchronize()
        if c["band"]:
            eng.set_band_width(c["band"])
            d = eng.describe(0, n)
            got = eng.score_device(0, d_reads, d_refs, stream=stream)
            if stream is not None:
                stream.synchronize()
            exp = cpu_ref.score_banded_sw(reads, refs, c["band"], osc, threads=8, block_rows=d["band_block_rows"], col_align=d["band_col_align"], affine=c["affine"])
            if not np.array_equal(got.cpu().numpy(), exp):
                return "banded score_device differs"
            # banded placed scores where the chain runs: refused with the key off, as ever; with band_placed = 1 against the
            # numpy restatement on the chain's band (tests/placed_band_ref.py: int64 cells, the record does not saturate)
            if d["band_block_rows"] == 16 and not c["policy"] and R * F * n <= 60_000_000:
                try:
                    eng.score_placed_device(0, d_reads, d_refs, stream=stream)
                    return "score_placed_device ran under a band with band_placed = 0"
                except hipkernel.HipKernelError as err:
                    if "band_width" not in str(err):
                        raise
                eng.set_band_placed(1)
                BAND_PLACED_CASES[0] += 1
                try:
                    eng.score_span_device(0, d_reads, d_refs, stream=stream)
                    return "score_span_device ran under a band"
                except hipkernel.HipKernelError as err:
                    if "band_width" not in str(err):
                        raise
                got = eng.score_placed_device(0, d_reads, d_refs, stream=stream)
                if stream is not None:
                    stream.synchronize()
                pexp = placed_band_ref.placed_banded(reads, refs, c["band"], osc, affine=c["affine"])
                if eng.describe(0, n)["ran_placed"] != "chain" or not np.array_equal(got.cpu().numpy().astype(np.int64), pexp):
                    return "banded score_placed_device differs (%s)" % eng.describe(0, n)["ran_placed"]
                if c["host"]:
                    h = eng.score_placed_host(0, reads, refs, threads=c["threads"])
                    if not np.array_equal(np.stack([h["score"], h["read_end"], h["ref_end"]], axis=1).astype(np.int64), pexp):
                        return "banded score_placed_host differs"
            # every other banded case also runs the NW variant under the band (band_nw = 1) against tests/band_nw_ref.py
            # (decided by the seed: no further draw, so the sequence of cases is the one it was)
            if c["seed"] % 2 and not c["policy"] and 2 * (c["band"] // 2) + 1 >= -(-F // R):
                NW_BAND_CASES[0] += 1
                eng.set_band_nw(1)
                eng.set_band_alignments(1)
                shape = (d["band_block_rows"], d["band_col_align"])
                got = eng.score_device(1, d_reads, d_refs, stream=stream)
                if stream is not None:
                    stream.synchronize()
                exp = np.minimum(band_nw_ref.score_banded_nw(reads, refs, c["band"], osc, *shape, affine=c["affine"]), 32767)
                if not np.array_equal(got.cpu().numpy().astype(np.int64), exp):
                    return "banded NW score_device differs"
                if R * F * n <= 30_000_000:
                    rows, idx = eng.align_device(1, d_reads, d_refs, stream=stream)
                    if stream is not None:
                        stream.synchronize()
                    e_rows, e_idx = band_nw_ref.align_banded_nw(reads, refs, c["band"], osc, *shape, affine=c["affine"])
                    if not (np.array_equal(rows.cpu().numpy(), e_rows) and np.array_equal(idx.cpu().numpy(), e_idx)):
                        return "banded NW align_device differs"
            return None
        for opt in ((0,) if c.get("subopt_only") else (0, 1)):
            exp = cpu_ref.score(opt, reads, refs, osc, threads=8, affine=c["affine"], wide=True)
            got = eng.score_device(opt, d_reads, d_refs, stream=stream)
            if stream is not None:
                stream.synchronize()
            if not np.array_equal(got.cpu().numpy(), exp):
                return "score_device opt %d differs" % opt
            if c["host"]:
                if not np.array_equal(eng.score_host(opt, reads, refs, threads=c["threads"]), exp):
                    return "score_host opt %d differs" % opt
            # placed scores: every case that runs Smith-Waterman scores unbanded under traceback_policy 0, against the numpy
            # restatement (tests/placed_ref.py: int64 cells -- a case whose cells could leave int16 must be refused instead)
            if opt == 0 and not c["policy"] and R * F * n <= 60_000_000:
                fits = min(R, F) * max(c["match"], 0) + 1 <= 32000
                try:
                    got = eng.score_placed_device(0, d_reads, d_refs, stream=stream)
                except hipkernel.HipKernelError:
                    if fits:
                        raise
                    got = None
                if got is not None:
                    if stream is not None:
                        stream.synchronize()
                    if not fits:
                        return "score_placed_device ran where the cells can leave int16"
                    PLACED_CASES[0] += 1
                    pexp = placed_ref.placed(reads, refs, osc, affine=c["affine"])
                    if not np.array_equal(got.cpu().numpy().astype(np.int64), pexp):
                        return "score_placed_device differs (%s)" % eng.describe(0, n)["ran_placed"]
                    if c["host"]:
                        h = eng.score_placed_host(0, reads, refs, threads=c["threads"])
                        if not np.array_equal(np.stack([h["score"], h["read_end"], h["ref_end"]], axis=1).astype(np.int64), pexp):
                            return "score_placed_host differs"
                    # suboptimal scores wherever placed scores ran on the register sweep: the numpy restatement, a mask
                    # decided by the seed (no further draw)
                    if eng.describe(0, n)["ran_placed"] in ("key", "rows"):
                        SUBOPT_CASES[0] += 1
                        mask = (0, 1, R // 2, R, F, c["seed"] % (F + 2))[c["seed"] % 6]
                        uexp = subopt_ref.subopt(reads, refs, osc, mask, affine=c["affine"])
                        got = eng.score_subopt_device(0, d_reads, d_refs, mask, stream=stream)
                        if stream is not None:
                            stream.synchronize()
                        if not np.array_equal(got.cpu().numpy().astype(np.int64), uexp):
                            return "score_subopt_device differs (%s, mask %d)" % (eng.describe(0, n)["ran_subopt"], mask)
                        if c["host"]:
                            h = eng.score_subopt_host(0, reads, refs, mask, threads=c["threads"])
                            if not np.array_equal(np.stack([h[k] for k in hipkernel.subopt_dtype().names], axis=1).astype(np.int64), uexp):
                                return "score_subopt_host differs (mask %d)" % mask
                    if c.get("subopt_only"):
                        continue
                    # spanned scores wherever placed scores ran: the numpy restatement, unclipped (tests/span_ref.py)
                    SPAN_CASES[0] += 1
                    sexp = span_ref.spans(reads, refs, osc, affine=c["affine"])
                    got = eng.score_span_device(0, d_reads, d_refs, stream=stream)
                    if stream is not None:
                        stream.synchronize()
                    if not np.array_equal(got.cpu().numpy().astype(np.int64), sexp):
                        return "score_span_device differs (%s)" % eng.describe(0, n)["ran_span"]
                    if c["host"]:
                        h = eng.score_span_host(0, reads, refs, threads=c["threads"])
                        if not np.array_equal(np.stack([h[k] for k in hipkernel.span_dtype().names], axis=1).astype(np.int64), sexp):
                            return "score_span_host differs"
        if R * F * n <= 30_000_000 and not c.get("subopt_only"):
            akw = dict(affine=True) if c["affine"] else dict(policy="sse" if c["policy"] else "default")
            for opt in (0, 1):
                e16 = cpu_ref.align(opt, reads, refs, osc, threads=8, **akw)
                e32 = cpu_ref.align(opt, reads, refs, osc, threads=8, wide=True, **akw)
                rows, idx = eng.align_device(opt, d_reads, d_refs, stream=stream)
                if stream is not None:
                    stream.synchronize()
                rows, idx = rows.cpu().numpy(), idx.cpu().numpy()
                ok = (np.array_equal(rows, e16[0]) and np.array_equal(idx, e16[1])) or (np.array_equal(rows, e32[0]) and np.array_equal(idx, e32[1]))
                if not ok:
                    return "align_device opt %d differs" % opt
                if c["host"]:
                    hrows, hidx = eng.align_host(opt, reads, refs, threads=c["threads"])
                    ok = (np.array_equal(hrows, e16[0]) and np.array_equal(hidx, e16[1])) or (np.array_equal(hrows, e32[0]) and np.array_equal(hidx, e32[1]))
                    if not ok:
                        return "align_host opt %d differs" % opt
        return None
    finally:
        if c["seed"] % 7:                  # (most engines are closed here; the rest are left to the finalizer / the atexit hook)
            eng.close()


def draw_span_cigar(rng):
    """--kind span_cigar: a shape the plain-Python walk of the reference can follow, a scoring, and the keys a spanned CIGAR call reads"""
    c = draw(rng, "subopt")
    if rng.random() < 0.5:
        c["R"], c["F"] = int(rng.integers(1, 321)), int(rng.integers(1, 901))
    if rng.random() < 0.125:
        c["R"], c["F"] = int(rng.integers(1025, 1400)), int(rng.integers(40, 1500))          # the row strips
    c["n"] = int(max(1, min(rng.integers(1, 200), 3_000_000 // max(c["R"] * c["F"], 1))))
    c.update(subopt_only=False, span_cigar=True, extended=bool(rng.random() < 0.5), stride=int(rng.choice([1, 2, 5, 64, 700])),
             ckpt=bool(rng.random() < 0.3), cap_mb=int(rng.integers(1, 8)) if rng.random() < 0.2 else 0, wide=bool(rng.random() < 0.2))
    return c


def run_span_cigar(c):
    R, F, n = c["R"], c["F"], c["n"]
    reads, refs = synth.make_pairs(n, R, F, seed=c["seed"], sub_rate=0.1, indel_rate=0.02, n_run_frac=0.1, short_frac=0.3, lowercase_frac=0.05, junk_frac=0.05)
    # a junk byte that happens to be '-' is a gap to the column rule (vh_cigar's, the encoders'): the ops would then consume one
    # base fewer than the span holds -- of the input's making, in the reference as in the library; not what this kind is after
    reads[reads == ord("-")] = ord("#")
    refs[refs == ord("-")] = ord("#")
    sc = hipkernel.Scoring.make(c["match"], c["mismatch"], c["gr"], c["gf"], **c["aff"])
    eng = hipkernel.Engine(R, F, sc)
    try:
        if c["ckpt"]:
            eng.set_trace_checkpoints(1)
        if c["cap_mb"]:
            eng.set_pointer_scratch_cap_mb(c["cap_mb"])
        if c["wide"]:
            eng.set_score_width(32)
            eng.set_placed_wide(1)
        stream = torch.cuda.Stream() if c["stream"] else None
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        torch.cuda.synchronize()
        exp = span_cigar_ref.expected(reads, refs, sc, affine=c["affine"], extended=c["extended"])
        recs = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
        ops = torch.full((n, c["stride"]), -7, dtype=torch.int32, device="cuda")
        eng.align_span_device(0, d_reads, d_refs, extended=c["extended"], ops_stride=c["stride"], stream=stream, out=(recs, ops))
        (stream or torch.cuda.current_stream()).synchronize()
        what = eng.describe(0, n)["ran_span_cigar"]
        if not np.array_equal(recs.cpu().numpy().astype(np.int64), exp["recs"]):
            return "align_span_device records differ (%s)" % what
        got = ops.cpu().numpy()
        for p in range(n):
            k = min(len(exp["ops"][p]), c["stride"])
            if got[p, :k].view(np.uint32).tolist() != exp["ops"][p][:k] or not (got[p, k:] == -7).all():
                return "align_span_device ops of pair %d differ (%s)" % (p, what)
        spans = eng.score_span_device(0, d_reads, d_refs, stream=stream)
        (stream or torch.cuda.current_stream()).synchronize()
        if not np.array_equal(spans.cpu().numpy().astype(np.int64), exp["spans"]):
            return "score_span_device after align_span_device differs"
        if c["host"]:
            h_recs, h_ops, offsets = eng.align_span_host(0, reads, refs, extended=c["extended"], threads=c["threads"])
            flat = np.stack([h_recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
            if not np.array_equal(flat, exp["recs"]) or h_ops.tolist() != [o for pair in exp["ops"] for o in pair]:
                return "align_span_host differs (%s)" % what
            if not np.array_equal(np.diff(offsets), exp["recs"][:, 5]):
                return "align_span_host offsets differ"
        return None
    finally:
        eng.close()


EXTEND_GEOMETRIES = [(0, 0), (8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32), (8, 4), (16, 12), (64, 24)]
EXTEND_FORMS = [(-3, -3), (-2, -4), (-3, -3, -5, -1, -5, -1), (-3, -3, -6, -2, -4, -1)]


def draw_extend_wide(rng):
    """an extend_wide = 1 case (a third of --kind extend): a long read that takes two to four 512-row strips, a scoring out of the
    signed int16 bound (match 970, or gaps of -320 and beyond), or score_width = 32 on an in-range call -- each on the int32 extension sweep"""
    why = ("long", "scoring", "width")[int(rng.integers(0, 3))]
    form = EXTEND_FORMS[int(rng.integers(0, 4))]
    match, scale, width = 2, 1, 0
    if why == "long":
        R, F, n = int(rng.integers(1025, 1600)), int(rng.integers(1, 301)), int(rng.integers(1, 10))
    else:
        R, F, n = int(rng.integers(1, 201)), int(rng.integers(1, 301)), int(rng.integers(1, 100))
    if why == "scoring":
        R, F = max(R, 34), max(F, 70)               # 34 x 970 and 104 gap steps at -320 or worse leave +-32000
        match, scale = ((970, 1), (2, 160))[int(rng.integers(0, 2))]
    if why == "width":
        width = 32
    return dict(R=R, F=F, n=n, scoring=(match, -int(rng.integers(1, 4))) + tuple(g * scale for g in form), affine=len(form) > 2, geometry=(0, 0),
                host=bool(rng.random() < 0.3), threads=int(rng.integers(1, 9)), seed=int(rng.integers(0, 1 << 30)), wide=why, width=width)


def draw_extend(rng):
    """--kind extend: a shape, a scoring inside the signed int16 bound (extend_choice, cell_rules.h: 500 gap steps at 60 stay above
    -32000), a geometry that holds the read, and whether the host entry runs too; a third of the cases are draw_extend_wide's"""
    if rng.random() < 1 / 3:
        return draw_extend_wide(rng)
    R, F = int(rng.integers(1, 201)), int(rng.integers(1, 301))
    match = int(rng.choice([1, 2, 3, 14, 60]))
    scale = {1: 1, 2: 1, 3: 1, 14: 4, 60: 10}[match]
    form = EXTEND_FORMS[int(rng.integers(0, 4))]
    fits = [gk for gk in EXTEND_GEOMETRIES if gk == (0, 0) or gk[0] * gk[1] >= R]
    return dict(R=R, F=F, n=int(rng.integers(1, 200)), scoring=(match, -int(rng.integers(1, match + 2))) + tuple(g * scale for g in form),
                affine=len(form) > 2, geometry=fits[int(rng.integers(0, len(fits)))], host=bool(rng.random() < 0.3), threads=int(rng.integers(1, 9)),
                seed=int(rng.integers(0, 1 << 30)))


def run_extend(c):
    """one extension-score case: the device entry (and, for some, the host entry) against tests/extend_ref.py, all five fields"""
    rng = np.random.default_rng(c["seed"])
    R, F, n = c["R"], c["F"], c["n"]
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = bases[rng.integers(0, 4, (n, R))], bases[rng.integers(0, 4, (n, F))]
    for p in range(n):
        if p % 3 < 2:                       # an extension from the anchor, a third of them behind extra reference bases
            L, shift = int(rng.integers(1, min(R, F) + 1)), (int(rng.integers(0, 3)) if p % 3 == 1 else 0)
            span = min(L, F - shift)
            if span > 0:
                refs[p, shift:shift + span] = reads[p, :span]
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.2:
            refs[p, int(rng.integers(0, F))] = rng.choice([0, ord("N"), 0x80, 0xFF])
    sc = hipkernel.Scoring.make(*c["scoring"])
    exp = extend_ref.extend(reads, refs, sc, affine=c["affine"], chunk=64 if R <= 200 else 4)
    eng = hipkernel.Engine(R, F, sc, group_lanes=c["geometry"][0], rows_per_lane=c["geometry"][1])
    try:
        if c.get("wide"):
            eng.set_extend_wide(1)
            eng.set_score_width(c["width"])
        got = eng.score_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        ran = eng.describe(0, n)["ran_extend"]
        if ran != ("wide" if c.get("wide") else "rows"):
            return "score_extend_device ran %s" % ran
        if not np.array_equal(got.cpu().numpy().astype(np.int64), exp):
            return "score_extend_device differs (%s)" % ran
        if c["host"]:
            h = eng.score_extend_host(0, reads, refs, threads=c["threads"])
            if not np.array_equal(np.stack([h[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64), exp):
                return "score_extend_host differs"
        return None
    finally:
        eng.close()


def draw_extend_band(rng):
    """--kind extend_band: a shape of one to four 512-row strips, a band from w = 0 to beyond the shape (the unbanded limit), one of
    the four gap forms, score_width 0 or 32, extend_wide 0 or 1, and whether the host entry runs too"""
    strips = int(rng.integers(1, 5))
    R = int(rng.integers(1, 201)) if strips == 1 and rng.random() < 0.5 else int(rng.integers(512 * (strips - 1) + 1, 512 * strips + 1))
    F = int(rng.integers(1, R + 400))
    band_width = int(rng.choice([1, 2, 3, int(rng.integers(1, 40)), int(rng.integers(1, 300)), int(rng.integers(1, 2 * max(R, F) + 40))]))
    form = EXTEND_FORMS[int(rng.integers(0, 4))]
    return dict(R=R, F=F, n=int(rng.integers(1, 12 if R > 512 else 60)), scoring=(2, -int(rng.integers(1, 4))) + form, affine=len(form) > 2, band_width=band_width,
                width=int(rng.choice([0, 32])), wide=int(rng.integers(0, 2)), host=bool(rng.random() < 0.3), threads=int(rng.integers(1, 9)),
                seed=int(rng.integers(0, 1 << 30)))


def run_extend_band(c):
    """one banded extension-score case: the device entry (and, for some, the host entry) against tests/extend_band_ref.py, all five
    fields.  The references are the reads with a few bases inserted -- fewer than w for some pairs, more than w + 8 for others --
    and ragged tails."""
    return run_extend_zdrop(dict(c, Z=0, banded=True))


def draw_extend_zdrop(rng):
    """--kind extend_zdrop: draw_extend_band's cases with a random Z -- small, of the scale of a read's score, never dropping -- and,
    for a third, without the band (the unbanded int32 sweep, whatever the read length)"""
    c = draw_extend_band(rng)
    c.update(Z=int(rng.choice([1, int(rng.integers(1, 40)), int(rng.integers(1, 400)), int(rng.integers(1, 4 * c["R"] + 2)), 1 << 29, 1 << 30])),
             banded=bool(rng.random() < 0.67))
    return c


def run_extend_zdrop(c):
    """one extension-score case under extend_zdrop = Z (Z = 0: a case of --kind extend_band): the device entry (and, for some, the
    host entry) against tests/extend_zdrop_ref.py -- all five fields and, on the device entry, the count of skipped waves.  Half of
    the pairs carry a run of A against C behind a random prefix, so that rows drop."""
    rng = np.random.default_rng(c["seed"])
    R, F, n, w = c["R"], c["F"], c["n"], c["band_width"] // 2
    Z, band_width = c["Z"], c["band_width"] if c["banded"] else 0
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = bases[rng.integers(0, 4, (n, R))], bases[rng.integers(0, 4, (n, F))]
    for p in range(n):
        d = int(rng.integers(0, max(w, 1))) if p % 2 == 0 else int(rng.integers(w + 9, w + 30))
        pos = int(rng.integers(0, max(1, min(R, F))))
        row = np.concatenate([reads[p, :pos], bases[rng.integers(0, 4, d)], reads[p, pos:]])[:F]
        refs[p, :len(row)] = row
        if Z and p % 4 < 2:
            a, g = int(rng.integers(0, R)), int(rng.integers(1, 40))
            reads[p, a:a + g] = ord("A")
            refs[p, a:a + g] = ord("C")
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.2:
            refs[p, int(rng.integers(0, F))] = rng.choice([0, ord("N"), 0x80, 0xFF])
    sc = hipkernel.Scoring.make(*c["scoring"])
    chunk = 64 if R <= 200 else 4
    if Z:
        exp, T = extend_zdrop_ref.extend(reads, refs, sc, Z, band_width, affine=c["affine"], chunk=chunk)
        skipped = extend_zdrop_ref.skipped_waves(T, extend_ref.trimmed_lengths(reads), extend_ref.trimmed_lengths(refs), R, band_width)
    else:
        exp, skipped = extend_band_ref.extend(reads, refs, sc, band_width, affine=c["affine"], chunk=chunk), 0
    route = "band" if band_width else "wide"
    eng = hipkernel.Engine(R, F, sc)
    try:
        eng.set_band_width(band_width)
        eng.set_extend_band(1 if band_width else 0)
        eng.set_score_width(c["width"])
        eng.set_extend_wide(c["wide"])
        eng.set_extend_zdrop(Z)
        got = eng.score_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        d = eng.describe(0, n)
        if d["ran_extend"] != route or d["ran_extend_zdrop"] != Z:
            return "score_extend_device ran %s under Z = %d" % (d["ran_extend"], d["ran_extend_zdrop"])
        if not np.array_equal(got.cpu().numpy().astype(np.int64), exp):
            return "score_extend_device differs (%s, Z = %d)" % (route, Z)
        if d["extend_zdrop_skipped_waves"] != skipped:
            return "skipped waves: %d, expected %d" % (d["extend_zdrop_skipped_waves"], skipped)
        if c["host"]:
            h = eng.score_extend_host(0, reads, refs, threads=c["threads"])
            if not np.array_equal(np.stack([h[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64), exp):
                return "score_extend_host differs (%s, Z = %d)" % (route, Z)
        return None
    finally:
        eng.close()


def draw_extend_zdrop_rows(rng):
    """--kind extend_zdrop_rows: draw_extend's register-sweep cases -- shapes up to the register limit, the four gap forms, the
    engine's own or a forced full geometry -- under extend_zdrop_rows = 1 with a random Z, as scores or, for half, as alignments with
    an end bonus"""
    c = None
    while c is None or c.get("wide"):
        c = draw_extend(rng)
    top = c["scoring"][0] * min(c["R"], c["F"])
    c.update(n=min(c["n"], 60), Z=int(rng.choice([1, 2, int(rng.integers(1, 40)), int(rng.integers(1, 400)), int(rng.integers(1, 4 * top + 2)), 1 << 29, 1 << 30])),
             align=bool(rng.random() < 0.5), bonus=int(rng.choice([-1, 0, int(rng.integers(0, top + 2)), 2 ** 31 - 1])), extended=bool(rng.random() < 0.5))
    return c


def run_extend_zdrop_rows(c):
    """one case of the register sweep's ZDROP instances: records (device, for some the host entry too) against
    tests/extend_zdrop_ref.py with band_width = 0, or alignments -- records, ops, extension records -- against
    tests/extend_align_ref.py on the reads cut at the reference's drop rows, a dropped pair from its best cell.  Half of the pairs
    carry a run of A against C, so that rows drop."""
    rng = np.random.default_rng(c["seed"])
    R, F, n, Z = c["R"], c["F"], c["n"], c["Z"]
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = bases[rng.integers(0, 4, (n, R))], bases[rng.integers(0, 4, (n, F))]
    for p in range(n):
        if p % 3 < 2:
            L, shift = int(rng.integers(1, min(R, F) + 1)), (int(rng.integers(0, 3)) if p % 3 == 1 else 0)
            span = min(L, F - shift)
            if span > 0:
                refs[p, shift:shift + span] = reads[p, :span]
        if p % 4 < 2:
            a, g = int(rng.integers(0, R)), int(rng.integers(1, 40))
            reads[p, a:a + g] = ord("A")
            refs[p, a:a + g] = ord("C")
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
    sc = hipkernel.Scoring.make(*c["scoring"])
    exp, T = extend_zdrop_ref.extend(reads, refs, sc, Z, 0, affine=c["affine"], chunk=64)
    eng = hipkernel.Engine(R, F, sc, group_lanes=c["geometry"][0], rows_per_lane=c["geometry"][1])
    try:
        eng.set_extend_zdrop(Z)
        eng.set_extend_zdrop_rows(1)
        d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
        if not c["align"]:
            got = eng.score_extend_device(0, d_reads, d_refs)
            torch.cuda.synchronize()
            d = eng.describe(0, n)
            if d["ran_extend"] != "rows" or d["ran_extend_zdrop"] != Z or d["extend_zdrop_skipped_waves"] != 0:
                return "score_extend_device ran %s under Z = %d" % (d["ran_extend"], d["ran_extend_zdrop"])
            if not np.array_equal(got.cpu().numpy().astype(np.int64), exp):
                return "score_extend_device differs (rows, Z = %d)" % Z
            if c["host"]:
                h = eng.score_extend_host(0, reads, refs, threads=c["threads"])
                if not np.array_equal(np.stack([h[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64), exp):
                    return "score_extend_host differs (rows, Z = %d)" % Z
            return None
        Rp = extend_ref.trimmed_lengths(reads)
        best, chosen = extend_align_ref.align(extend_zdrop_ref.cut_reads(reads, T), refs, sc, c["affine"], end_bonus=(-1, c["bonus"]), extended=c["extended"])
        dropped = T < Rp
        exp_recs = np.where(dropped[:, None], best[0], chosen[0])
        exp_ops = [best[1][k] if dropped[k] else chosen[1][k] for k in range(n)]
        stride = max([len(o) for o in exp_ops] + [1]) + 1
        recs, ops, ext = eng.align_extend_device(0, d_reads, d_refs, end_bonus=c["bonus"], extended=c["extended"], ops_stride=stride)
        torch.cuda.synchronize()
        d = eng.describe(0, n)
        if d["ran_extend_align"] != "rows" or d["ran_extend_zdrop"] != Z:
            return "align_extend_device ran %s under Z = %d" % (d["ran_extend_align"], d["ran_extend_zdrop"])
        if not np.array_equal(recs.cpu().numpy().astype(np.int64), exp_recs):
            return "align_extend_device: records differ (Z = %d)" % Z
        got_ops = ops.cpu().numpy().view(np.uint32)
        for k, want in enumerate(exp_ops):
            if got_ops[k, :len(want)].tolist() != want:
                return "align_extend_device: ops of pair %d differ (Z = %d)" % (k, Z)
        if not np.array_equal(ext.cpu().numpy().astype(np.int64), exp):
            return "align_extend_device: extension records differ (Z = %d)" % Z
        return None
    finally:
        eng.close()


def draw_extend_align(rng):
    """--kind extend_align: draw_extend's register-sweep cases (shape, scoring inside the signed int16 bound, the engine's own or a
    forced full geometry) with an end bonus -- none, zero, small, of the scale of the scores, or "always the read end" --, extended,
    an ops_stride that some alignments overflow, and a pointer-scratch cap for some"""
    c = None
    while c is None or c.get("wide"):
        c = draw_extend(rng)
    top = c["scoring"][0] * min(c["R"], c["F"])
    c.update(n=min(c["n"], 60), bonus=int(rng.choice([-1, -1, 0, int(rng.integers(1, 12)), int(rng.integers(0, top + 2)), 2 ** 31 - 1, 2 ** 31 - 1])),
             extended=bool(rng.random() < 0.5), stride=int(rng.choice([1, 2, 5, 64, 700])), cap_mb=int(rng.integers(1, 4)) if rng.random() < 0.2 else 0,
             with_extend=bool(rng.random() < 0.7))
    return c


def run_extend_align(c):
    """one extension-alignment case: the device entry (and, for some, the host entry) against tests/extend_align_ref.py -- records,
    the stored ops with the sentinel behind them untouched, and the extension records"""
    rng = np.random.default_rng(c["seed"])
    R, F, n = c["R"], c["F"], c["n"]
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = bases[rng.integers(0, 4, (n, R))], bases[rng.integers(0, 4, (n, F))]
    for p in range(n):
        if p % 3 < 2:                       # an extension from the anchor, a third of them behind extra reference bases
            L, shift = int(rng.integers(1, min(R, F) + 1)), (int(rng.integers(0, 3)) if p % 3 == 1 else 0)
            span = min(L, F - shift)
            if span > 0:
                refs[p, shift:shift + span] = reads[p, :span]
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.2:
            refs[p, int(rng.integers(0, F))] = rng.choice([0, ord("N"), 0x80, 0xFF])
    sc = hipkernel.Scoring.make(*c["scoring"])
    exp_recs, exp_ops, exp_ext, _ = extend_align_ref.align(reads, refs, sc, c["affine"], end_bonus=c["bonus"], extended=c["extended"])
    eng = hipkernel.Engine(R, F, sc, group_lanes=c["geometry"][0], rows_per_lane=c["geometry"][1])
    try:
        if c["cap_mb"]:
            eng.set_pointer_scratch_cap_mb(c["cap_mb"])
        stride = c["stride"]
        recs = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
        ops = torch.full((n, stride), -7, dtype=torch.int32, device="cuda")
        ext = torch.full((n, 5), -7, dtype=torch.int32, device="cuda") if c["with_extend"] else None
        eng.align_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), end_bonus=c["bonus"], extended=c["extended"],
                                ops_stride=stride, out=(recs, ops, ext))
        torch.cuda.synchronize()
        if eng.describe(0, n)["ran_extend_align"] != "rows":
            return "align_extend_device ran %s" % eng.describe(0, n)["ran_extend_align"]
        if not np.array_equal(recs.cpu().numpy().astype(np.int64), exp_recs):
            return "align_extend_device: records differ"
        got = ops.cpu().numpy()
        for p, want in enumerate(exp_ops):
            k = min(len(want), stride)
            if got[p, :k].view(np.uint32).tolist() != want[:k] or not (got[p, k:] == -7).all():
                return "align_extend_device: ops of pair %d differ" % p
        if ext is not None and not np.array_equal(ext.cpu().numpy().astype(np.int64), exp_ext):
            return "align_extend_device: extension records differ"
        if c["host"]:
            h_recs, h_ops, offsets, h_ext = eng.align_extend_host(0, reads, refs, end_bonus=c["bonus"], extended=c["extended"],
                                                                  with_extend=c["with_extend"], threads=c["threads"])
            flat = np.stack([h_recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
            if not np.array_equal(flat, exp_recs) or h_ops.tolist() != [o for pair in exp_ops for o in pair]:
                return "align_extend_host differs"
            if h_ext is not None and not np.array_equal(np.stack([h_ext[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64), exp_ext):
                return "align_extend_host: extension records differ"
        return None
    finally:
        eng.close()


def draw_extend_band_align(rng):
    """--kind extend_band_align: draw_extend_band's cases (one to four 512-row strips, random bands up to the unbanded limit, four
    gap forms, ragged tails) with one of three end bonuses -- the best cell, "the read end wherever it is reached", 20 --, extended,
    an ops_stride that some alignments overflow, and a pointer-scratch cap for some"""
    c = draw_extend_band(rng)
    c.update(n=min(c["n"], 8 if c["R"] > 512 else 24), bonus=int(rng.choice([-1, 2 ** 31 - 1, 20])), extended=bool(rng.random() < 0.5),
             stride=int(rng.choice([1, 5, 64, 3000])), cap_mb=1 if rng.random() < 0.3 else 0, with_extend=bool(rng.random() < 0.7))
    return c


def run_extend_band_align(c):
    """one banded extension-alignment case: the device entry (and, for some, the host entry) against
    tests/extend_band_align_ref.py -- records, the stored ops with the sentinel behind them untouched, and the extension records.
    The references are the reads with a few bases inserted -- fewer than w for some pairs, more than w + 8 for others -- and ragged
    tails; no literal '-' byte (the caveat of every CIGAR call)."""
    rng = np.random.default_rng(c["seed"])
    R, F, n, w = c["R"], c["F"], c["n"], c["band_width"] // 2
    bases = np.frombuffer(b"ACGT", np.uint8)
    reads, refs = bases[rng.integers(0, 4, (n, R))], bases[rng.integers(0, 4, (n, F))]
    for p in range(n):
        d = int(rng.integers(0, max(w, 1))) if p % 2 == 0 else int(rng.integers(w + 9, w + 30))
        pos = int(rng.integers(0, max(1, min(R, F))))
        row = np.concatenate([reads[p, :pos], bases[rng.integers(0, 4, d)], reads[p, pos:]])[:F]
        refs[p, :len(row)] = row
        if rng.random() < 0.3:
            reads[p, int(rng.integers(0, R + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.3:
            refs[p, int(rng.integers(0, F + 1)):] = rng.choice([0, ord("N")])
        if rng.random() < 0.2:
            refs[p, int(rng.integers(0, F))] = rng.choice([0, ord("N"), 0x80, 0xFF])
    sc = hipkernel.Scoring.make(*c["scoring"])
    exp_recs, exp_ops, exp_ext, _, _ = extend_band_align_ref.align(reads, refs, sc, c["band_width"], c["affine"], end_bonus=c["bonus"], extended=c["extended"],
                                                                   chunk=16 if R <= 200 else 2)
    eng = hipkernel.Engine(R, F, sc)
    try:
        eng.set_band_width(c["band_width"])
        eng.set_extend_band(1)
        eng.set_extend_band_align(1)
        eng.set_score_width(c["width"])
        eng.set_extend_wide(c["wide"])
        if c["cap_mb"]:
            eng.set_pointer_scratch_cap_mb(c["cap_mb"])
        stride = c["stride"]
        recs = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
        ops = torch.full((n, stride), -7, dtype=torch.int32, device="cuda")
        ext = torch.full((n, 5), -7, dtype=torch.int32, device="cuda") if c["with_extend"] else None
        eng.align_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), end_bonus=c["bonus"], extended=c["extended"],
                                ops_stride=stride, out=(recs, ops, ext))
        torch.cuda.synchronize()
        if eng.describe(0, n)["ran_extend_align"] != "band":
            return "align_extend_device ran %s" % eng.describe(0, n)["ran_extend_align"]
        if not np.array_equal(recs.cpu().numpy().astype(np.int64), exp_recs):
            return "align_extend_device (band): records differ"
        got = ops.cpu().numpy()
        for p, want in enumerate(exp_ops):
            k = min(len(want), stride)
            if got[p, :k].view(np.uint32).tolist() != want[:k] or not (got[p, k:] == -7).all():
                return "align_extend_device (band): ops of pair %d differ" % p
        if ext is not None and not np.array_equal(ext.cpu().numpy().astype(np.int64), exp_ext):
            return "align_extend_device (band): extension records differ"
        if c["host"]:
            h_recs, h_ops, offsets, h_ext = eng.align_extend_host(0, reads, refs, end_bonus=c["bonus"], extended=c["extended"],
                                                                  with_extend=c["with_extend"], threads=c["threads"])
            flat = np.stack([h_recs[k] for k in hipkernel.aln_dtype().names], axis=1).astype(np.int64)
            if not np.array_equal(flat, exp_recs) or h_ops.tolist() != [o for pair in exp_ops for o in pair]:
                return "align_extend_host differs (band)"
            if h_ext is not None and not np.array_equal(np.stack([h_ext[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64), exp_ext):
                return "align_extend_host (band): extension records differ"
        return None
    finally:
        eng.close()


def soak_sequences(rng, a):
    """--kind sequence: the generator and the runner of tests/engine_sequences.py (what tests/test_gpu_engine_sequences.py runs
    on its committed seeds) on random seeds: ONE engine per sequence through changes of all fifteen keys (extend_wide, extend_band
    and extend_band_align among them) and calls of all nine families -- spanned CIGARs, extension scores and extension alignments
    included, with their end_bonus, with_extend and extended, on the register route, the int32 sweep and the BANDED strip sweep --,
    every call against the reference of the route the state selects and against a new engine.  The worlds are the three with
    committed seeds (12 x 20, 150 x 200, 1 600 x 96); the 520 x 600 world of the hand-written sequences has no generated ones.
    No code path of its own: a mismatch is the runner's, with world, seed and step index."""
    os.environ["VALIGN_HIP_DEBUG"] = "ragged_min=8"        # (before any engine exists: the length classes at these batch sizes)
    import engine_sequences as es
    runners, t0, done = {}, time.time(), 0
    worlds = sorted(world for world in es.WORLDS if es.WORLDS[world]["seeds"])
    while time.time() - t0 < a.seconds:
        world = str(rng.choice(worlds))
        scoring = str(rng.choice(es.WORLDS[world]["scorings"]))
        seed = int(rng.integers(10, 1 << 30))
        if (world, scoring) not in runners:
            runners[(world, scoring)] = es.Runner(world, scoring)
        try:
            stats = runners[(world, scoring)].run(seed, log=print if a.verbose else None)
        except AssertionError as e:               # (es.SequenceMismatch is one; so are the references' own checks)
            print("MISMATCH world %s scoring %s seed %d: %s" % (world, scoring, seed, e), flush=True)
            return 1
        done += 1
        print("%s %s seed %d: %d calls, %d refused; %d sequences, %.0f s" % (world, scoring, seed, stats["calls"], stats["refused"], done,
                                                                              time.time() - t0), flush=True)
    print("ok: %d sequences in %.0f s (seed %d)" % (done, time.time() - t0, a.seed))
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=120.0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--kind", choices=["subopt", "sequence", "span_cigar", "extend", "extend_band", "extend_zdrop", "extend_zdrop_rows", "extend_align", "extend_band_align"], default=None,
                    help="draw cases of this kind only (default: the mix); sequence: one engine through tests/engine_sequences.py's sequences "
                         "(fifteen keys, extend_band and extend_band_align among them; nine families of calls, the banded extension routes included)")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    if a.kind == "sequence":
        return soak_sequences(rng, a)
    t0 = time.time()
    i = done = 0
    while time.time() - t0 < a.seconds:
        own = {"span_cigar": (draw_span_cigar, run_span_cigar), "extend": (draw_extend, run_extend), "extend_band": (draw_extend_band, run_extend_band), "extend_align": (draw_extend_align, run_extend_align),
               "extend_band_align": (draw_extend_band_align, run_extend_band_align), "extend_zdrop": (draw_extend_zdrop, run_extend_zdrop),
               "extend_zdrop_rows": (draw_extend_zdrop_rows, run_extend_zdrop_rows)}.get(a.kind)
        c = own[0](rng) if own else draw(rng, a.kind)
        if i >= a.first:
            if a.verbose:
                print("case %d: %r" % (i, c), flush=True)
            try:
                err = own[1](c) if own else run(c)
            except hipkernel.HipKernelError as e:
                err = "library error: %s" % e
            done += 1
            if err:
                print("MISMATCH case %d (seed %d): %s\n  %r" % (i, a.seed, err, c), flush=True)
                return 1
            if done % 25 == 0:
                print("%d cases, %.0f s" % (done, time.time() - t0), flush=True)
        i += 1
    print("ok: %d cases in %.0f s (seed %d), %d of them with the banded NW variant, %d with placed scores, %d with spanned scores, "
          "%d with suboptimal scores, %d with banded placed scores" % (done, time.time() - t0, a.seed, NW_BAND_CASES[0], PLACED_CASES[0], SPAN_CASES[0],
                                                                        SUBOPT_CASES[0], BAND_PLACED_CASES[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
