"""The compact result format (include/valign_hip.h: valign_hip_aln + 32-bit ops) restated for the tests, from the ORACLE's
rows (cpu_ref.align / band_align_ref), never from the library's own output.

  ops ........... plain Python: the column rule of vh_cigar ('-' in the read row only is D, '-' in the ref row only is I, else
                  M, or extended '=' where the bytes are equal ignoring case and X where not) and the run lengths, one
                  `length << 4 | code` per run with the BAM codes M 0, I 1, D 2, = 7, X 8;
  text .......... host.cigars (vh_cigar) of the same rows;
  score ......... band_align_ref.rescore;
  end cells ..... independently of the code under test: Smith-Waterman from band_align_ref.align_banded_sw with a band wider
                  than the matrix (paths=True: the first walked cell is the end cell), the NW variant from
                  ckpt_align_ref._forward's end cell.  Both are plain Python / numpy and state the Default tie-breaks only.
  properties .... what pins the coordinates where no independent end cell is to hand: the degapped rows are
                  read[read_begin:read_end] / ref[ref_begin:ref_end].
"""
import numpy as np

import band_align_ref
import ckpt_align_ref
from versalignlib_amd import host

M, I, D, EQ, X = 0, 1, 2, 7, 8
LETTER = {M: "M", I: "I", D: "D", EQ: "=", X: "X"}
GAP = ord("-")


def ops_of_rows(rows, idx, extended=False):
    """-> per pair the list of ops (ints) of the alignment in rows [n, 2, AL] / idx [n, 4]."""
    out = []
    for p in range(len(rows)):
        s, e = int(idx[p, 0]) & 0xFFFF, int(idx[p, 1]) & 0xFFFF
        ops, run, op = [], 0, None
        for a, b in zip(rows[p, 0, s:e].tolist(), rows[p, 1, s:e].tolist()):
            if a == 0 and b == 0:
                break
            if a == GAP and b != GAP:
                now = D
            elif b == GAP and a != GAP:
                now = I
            elif not extended:
                now = M
            else:
                now = EQ if (a | 0x20) == (b | 0x20) else X
            if run and now != op:
                ops.append(run << 4 | op)
                run = 0
            op = now
            run += 1
        if run:
            ops.append(run << 4 | op)
        out.append(ops)
    return out


def text_of_ops(ops):
    """plain Python rendering (the library's is host.cigar_text)"""
    return "".join("%d%s" % (int(o) >> 4, LETTER[int(o) & 15]) for o in ops)


def degapped(rows, idx):
    """-> per pair (read bases, ref bases) of the alignment as bytes"""
    out = []
    for p in range(len(rows)):
        s, e = int(idx[p, 0]) & 0xFFFF, int(idx[p, 1]) & 0xFFFF
        a, b = rows[p, 0, s:e], rows[p, 1, s:e]
        out.append((a[(a != GAP) & (a != 0)].tobytes(), b[(b != GAP) & (b != 0)].tobytes()))
    return out


def end_cells_sw(reads, refs, scoring, affine=False):
    """-> int array [n, 2]: (read_pos, ref_pos) of the Smith-Waterman end cell (Default rules), -1 -1 for an empty alignment"""
    R, F = reads.shape[1], refs.shape[1]
    _, _, walked = band_align_ref.align_banded_sw(reads, refs, 2 * max(R, F) + 2, scoring, affine=affine, paths=True)
    return np.array([w[0] if w else (-1, -1) for w in walked], np.int64).reshape(len(reads), 2)


def end_cells_nw(reads, refs, scoring, affine=False):
    """... of the NW variant (Default rules), plain Python: small shapes / few pairs only"""
    tab = ckpt_align_ref._subst(scoring).tolist()
    out = []
    for p in range(len(reads)):
        rc = ckpt_align_ref._CLASS[reads[p]].tolist()
        fc = ckpt_align_ref._CLASS[refs[p]].tolist()
        _, i, j = ckpt_align_ref._forward(ckpt_align_ref.NW, affine, scoring, tab, rc, fc, len(rc))
        out.append((i, j))
    return np.array(out, np.int64).reshape(len(reads), 2)


def expected(rows, idx, scoring, reads, refs, extended=False, affine=False, ends=None):
    """What the library must return for the alignments rows / idx (the oracle's): a dict of
    ops (list of lists), text (host.cigars), n_ops, score, and -- with `ends` [n, 2], the independent end cells --
    begin / end coordinates [n, 4] = read_begin, read_end, ref_begin, ref_end."""
    ops = ops_of_rows(rows, idx, extended)
    exp = {"ops": ops, "text": host.cigars(rows, idx, extended=extended), "n_ops": np.array([len(o) for o in ops], np.int64),
           "score": band_align_ref.rescore(rows, idx, scoring, affine=affine), "bases": degapped(rows, idx)}
    assert [text_of_ops(o) for o in ops] == exp["text"]          # the two statements of the format agree on the oracle's rows
    if ends is not None:
        coords = np.zeros((len(rows), 4), np.int64)
        for p, (a, b) in enumerate(exp["bases"]):
            if not ops[p]:
                continue                                        # the empty alignment: all zeros
            re_, fe = int(ends[p, 0]) + 1, int(ends[p, 1]) + 1
            coords[p] = (re_ - len(a), re_, fe - len(b), fe)
        exp["coords"] = coords
    return exp


def check(recs, ops_of_pair, exp, reads, refs, what=""):
    """recs: structured array (hipkernel.aln_dtype) [n]; ops_of_pair(p) -> the pair's stored ops (uint32 array)."""
    n = len(recs)
    for p in range(n):
        got = [int(x) for x in ops_of_pair(p)]
        assert int(recs["n_ops"][p]) == exp["n_ops"][p], (what, p, "n_ops", int(recs["n_ops"][p]), exp["n_ops"][p])
        assert got == exp["ops"][p], (what, p, "ops", text_of_ops(got), exp["text"][p])
        assert host.cigar_text(np.array(got, np.uint32)) == exp["text"][p], (what, p, "text")
        assert int(recs["score"][p]) == int(exp["score"][p]), (what, p, "score", int(recs["score"][p]), int(exp["score"][p]))
        rb, re_, fb, fe = (int(recs[k][p]) for k in ("read_begin", "read_end", "ref_begin", "ref_end"))
        if "coords" in exp:
            assert (rb, re_, fb, fe) == tuple(int(x) for x in exp["coords"][p]), (what, p, "coords", (rb, re_, fb, fe), exp["coords"][p])
        if not exp["ops"][p]:
            assert (rb, re_, fb, fe, int(recs["score"][p])) == (0, 0, 0, 0, 0), (what, p, "empty alignment")
            continue
        assert 0 <= rb <= re_ <= reads.shape[1] and 0 <= fb <= fe <= refs.shape[1], (what, p, "range", (rb, re_, fb, fe))
        a, b = exp["bases"][p]
        assert reads[p, rb:re_].tobytes() == a and refs[p, fb:fe].tobytes() == b, (what, p, "degapped rows", (rb, re_, fb, fe))
