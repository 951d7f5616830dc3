"""Spanned CIGARs (include/valign_hip.h: valign_hip_align_span_*) restated in numpy / plain Python, independent of the library
and of the oracle's C, and UNCLIPPED: the alignment runs over the whole reversed prefixes.

  coordinates ... span_ref.spans: score, read_begin, read_end, ref_begin, ref_end.
  alignment ..... the Default Smith-Waterman alignment of the reversed prefixes read[0, read_end) and ref[0, ref_end)
                  (span_ref._reversed_prefixes; band_align_ref.align_banded_sw with a band wider than the matrix, plain Python
                  walk, Default tie-breaks), its columns reversed: the alignment in forward reading order.
  ops ........... cigar_ref.ops_of_rows of the reversed rows (vh_cigar's column rule and run lengths).
  score ......... band_align_ref.rescore of the reversed rows.

`walked` are the cells of the reversed matrix the walk emitted, first to last: walked[0] is the reversed end cell -- the
spanned begin cell --, walked[-1] the cell where the walk ended."""
import functools

import numpy as np

import band_align_ref
import cigar_ref
import span_ref

GAP = ord("-")


def reversed_alignments(reads, refs, spans, scoring, affine=False):
    """-> rows uint8 [n, 2, R + F] and idx int16 [n, 4] of the alignments of the reversed prefixes, their columns put back in
    forward reading order (same window idx[0] .. idx[1]), and the walked cells of the reversed matrix"""
    reads = np.asarray(reads, np.uint8)
    refs = np.asarray(refs, np.uint8)
    R, F = reads.shape[1], refs.shape[1]
    rr = span_ref._reversed_prefixes(reads, spans[:, 2])
    rf = span_ref._reversed_prefixes(refs, spans[:, 4])
    rows, idx, walked = band_align_ref.align_banded_sw(rr, rf, 2 * max(R, F) + 2, scoring, affine=affine, paths=True)
    fwd = np.zeros_like(rows)
    for p in range(len(rows)):
        s, e = int(idx[p, 0]), int(idx[p, 1])
        fwd[p, :, s:e] = rows[p, :, s:e][:, ::-1]
    return fwd, idx, walked


def expected(reads, refs, scoring, affine=False, extended=False):
    """What valign_hip_align_span_* must return: a dict of spans int64 [n, 5] (span_ref.spans), recs int64 [n, 6] (read_begin,
    read_end, ref_begin, ref_end, score, n_ops), ops (list of lists), rows / idx / walked (the alignment behind them)."""
    spans = span_ref.spans(reads, refs, scoring, affine=affine, chunk=32)
    rows, idx, walked = reversed_alignments(reads, refs, spans, scoring, affine)
    ops = cigar_ref.ops_of_rows(rows, idx, extended)
    score = band_align_ref.rescore(rows, idx, scoring, affine=affine)
    recs = np.zeros((len(reads), 6), np.int64)
    hit = spans[:, 0] > 0
    recs[:, 0:4] = np.where(hit[:, None], spans[:, 1:5], 0)
    recs[:, 4] = np.where(hit, score, 0)
    recs[:, 5] = [len(o) if h else 0 for o, h in zip(ops, hit)]
    ops = [o if h else [] for o, h in zip(ops, hit)]
    return {"spans": spans, "recs": recs, "ops": ops, "rows": rows, "idx": idx, "walked": walked}


@functools.lru_cache(maxsize=None)
def case(R, F, form, seed=None, n=64, extended=False):
    """The shared inputs of the CPU and the GPU tests, computed once a process: span_cases.pairs(n, R, F, seed) (seed
    11 * R + F unless given) under span_cases.scoring(form) -> (reads, refs, expected(...)); nothing of it is to be written to"""
    import span_cases
    reads, refs = span_cases.pairs(n, R, F, 11 * R + F if seed is None else seed)
    exp = expected(reads, refs, span_cases.scoring(form), affine=span_cases.is_affine(form), extended=extended)
    for a in (exp["spans"], exp["recs"], exp["rows"], exp["idx"]):
        a.setflags(write=False)
    return reads, refs, exp


def consumed(ops):
    """-> (read bases, reference bases) the ops consume"""
    read = sum(int(o) >> 4 for o in ops if (int(o) & 15) in (cigar_ref.M, cigar_ref.I, cigar_ref.EQ, cigar_ref.X))
    ref = sum(int(o) >> 4 for o in ops if (int(o) & 15) in (cigar_ref.M, cigar_ref.D, cigar_ref.EQ, cigar_ref.X))
    return read, ref


def has_gap(ops):
    return any((int(o) & 15) in (cigar_ref.I, cigar_ref.D) for o in ops)
