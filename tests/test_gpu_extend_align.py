"""Extension alignments on the GPU (valign_hip_align_extend_device / _host): records, ops and extension records against
tests/extend_align_ref.py (numpy / Python, int64 cells, the whole matrix, the walk on cell values, independent of the library).
Integers, compared exactly."""
import ctypes

import numpy as np
import pytest
import torch

import extend_align_ref as ref
import instance_matrix as im
from conftest import debug_switches
from test_gpu_extend import _batch
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]
FORMS = {"lin": (-2, -4), "aff": (-3, -3, -6, -2, -4, -1), "affsym": (-3, -3, -5, -1, -5, -1), "aff open == ext": (-3, -3, -2, -2, -1, -1)}
BASES = np.frombuffer(b"ACGT", np.uint8)
ALWAYS = ref.INT32_MAX


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _affine(form):
    return len(FORMS[form]) > 2


def _stride(exp):
    return max([len(o) for res in exp for o in res[1]] + [1]) + 2


def _run(eng, reads, refs, bonus, extended=False, stride=64, with_extend=True, opt=0):
    recs, ops, ext = eng.align_extend_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), end_bonus=bonus, extended=extended,
                                             ops_stride=stride, with_extend=with_extend)
    torch.cuda.synchronize()
    return recs.cpu().numpy().astype(np.int64), ops.cpu().numpy().view(np.uint32), None if ext is None else ext.cpu().numpy().astype(np.int64)


def _check(got, exp, what):
    recs, ops, ext = got
    exp_recs, exp_ops, exp_ext, _ = exp
    bad = np.nonzero((recs != exp_recs).any(axis=1))[0]
    assert bad.size == 0, (what, "records of pairs", bad[:8].tolist(), "got", recs[bad[:4]].tolist(), "expected", exp_recs[bad[:4]].tolist())
    for p, want in enumerate(exp_ops):
        assert ops[p, :len(want)].tolist() == want, (what, "ops of pair", p, ops[p, :len(want)].tolist(), want)
    if ext is not None:
        bad = np.nonzero((ext != exp_ext).any(axis=1))[0]
        assert bad.size == 0, (what, "extension records of pairs", bad[:8].tolist(), ext[bad[:4]].tolist(), exp_ext[bad[:4]].tolist())


def _same(a, b, what):
    """two device results: records, the stored ops and the extension records"""
    assert (a[0] == b[0]).all(), (what, "records", np.nonzero((a[0] != b[0]).any(axis=1))[0][:8].tolist())
    stored = np.arange(a[1].shape[1])[None, :] < np.minimum(a[0][:, 5], a[1].shape[1])[:, None]
    assert (a[1][stored] == b[1][stored]).all(), (what, "ops")
    assert (a[2] is None) == (b[2] is None) and (a[2] is None or (a[2] == b[2]).all()), (what, "extension records")


# ---- 1. every compiled instance: six full geometries x {linear, affine}, at the instance matrix's shapes, from both kinds of end ----
@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("G,K", FULL)
def test_every_instance(G, K, shape):
    n = im.batch(G)
    R, F = im.shapes(G, K)[shape]
    reads, refs = _batch(n, R, F, seed=G * K + shape)
    for form in ("lin", "aff"):
        sc = _scoring(form)
        exp = ref.align(reads, refs, sc, _affine(form), end_bonus=(-1, ALWAYS), chunk=16)
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        for bonus, want in zip((-1, ALWAYS), exp):
            _check(_run(eng, reads, refs, bonus, stride=_stride(exp)), want, (G, K, R, F, form, bonus))
            d = eng.describe(0, n)
            assert d["ran_extend_align"] == "rows" and d["ran_extend_align_geometry"] == "%dx%d" % (G, K), (G, K, R, F, form, d)
        eng.close()
        assert any(e is not None for e in exp[0][3]) and all(e is None or e[0] + 1 == rp for e, rp in zip(exp[1][3], ref.trimmed_lengths(reads)))


# ---- 2. pointer-block edges: 16 x 10, 24 steps (an exact last block) and 25 (a block that holds one step) ----
@pytest.mark.parametrize("F", [9, 10])
@pytest.mark.parametrize("R", [160, 149])
def test_pointer_block_edges(R, F):
    G, K = 16, 10
    assert F + G - 1 == {9: 24, 10: 25}[F]
    n = im.batch(G)
    reads, refs = _batch(n, R, F, seed=F, trim=False)
    refs[::3, :] = reads[::3, R - F:]               # the last column holds a base of every pair, and some paths run through the last rows
    for form in ("lin", "aff"):
        sc = _scoring(form)
        exp = ref.align(reads, refs, sc, _affine(form), end_bonus=(-1, ALWAYS), extended=True)
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        for bonus, want in zip((-1, ALWAYS), exp):
            _check(_run(eng, reads, refs, bonus, extended=True, stride=_stride(exp)), want, (R, F, form, bonus))
        eng.close()
        assert any(e is not None and e[1] == F - 1 for e in exp[1][3])          # a walk starts in the last swept column


# ---- 3. the bonus rule in between: some pairs end at the read end, the others at the best cell ----
@pytest.mark.parametrize("form", ["lin", "affsym"])
def test_bonus_between(form):
    G, K, R, F, bonus = 8, 8, 55, 23, 20
    n = im.batch(G)
    assert n == 73
    reads, refs = _batch(n, R, F, seed=G * K + 3)
    sc = _scoring(form)
    exp = ref.align(reads, refs, sc, _affine(form), end_bonus=bonus)
    Rp = ref.trimmed_lengths(reads)
    at_read_end = sum(1 for p in range(n) if Rp[p] > 0 and exp[2][p, 3] + bonus >= exp[2][p, 0])
    assert at_read_end >= 8 and sum(1 for p in range(n) if exp[3][p] is not None) - at_read_end >= 8
    eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
    _check(_run(eng, reads, refs, bonus, stride=_stride([exp])), exp, (form, bonus))
    eng.close()


# ---- 4. planted borders ----
def _planted(R, F):
    rng = np.random.default_rng(R * F + 1)
    reads, refs, names = [], [], []

    def add(name, rd, rf):
        assert len(rd) == R and len(rf) == F
        reads.append(np.asarray(rd, np.uint8))
        refs.append(np.asarray(rf, np.uint8))
        names.append(name)

    core = BASES[rng.integers(0, 4, R)]
    other = BASES[(np.searchsorted(BASES, core) + 1) % 4]
    junk = np.full(F, ord("T"), np.uint8)
    follow = junk.copy()
    follow[:min(R, F)] = core[:min(R, F)]
    add("Rp 0 (NUL)", np.zeros(R, np.uint8), follow)
    add("Rp 0 (N)", np.full(R, ord("N"), np.uint8), follow)
    add("Fp 0", core, np.full(F, ord("N"), np.uint8))
    rd = np.zeros(R, np.uint8)
    rd[:R // 2] = core[:R // 2]
    add("Fp 0, short read", rd, np.zeros(F, np.uint8))
    for extra in (1, 3):
        rf = junk.copy()                            # the reference begins with extra bases: a first op D
        rf[:extra] = other[:extra]
        rf[extra:extra + min(R, F - extra)] = core[:min(R, F - extra)]
        add("first D %d" % extra, core, rf)
        rd = core.copy()                            # the read begins with extra bases: a first op I
        rf = junk.copy()
        rf[:min(R - extra, F)] = core[extra:extra + min(R - extra, F)]
        rd[:extra] = BASES[(np.searchsorted(BASES, rf[:extra]) + 2) % 4]
        add("first I %d" % extra, rd, rf)
    add("all mismatch", np.full(R, ord("A"), np.uint8), np.full(F, ord("C"), np.uint8))
    for Rp, Fp in ((R, F), (R, min(R, F) // 2), (R // 2, F), (R // 3, R // 3), (2, 1), (1, 2)):
        rd, rf = np.full(R, ord("N"), np.uint8), np.zeros(F, np.uint8)      # homopolymers: DIAG, UP and LEFT tie along the way
        rd[:Rp] = ord("A")
        rf[:Fp] = ord("A")
        add("homopolymer %d x %d" % (Rp, Fp), rd, rf)
    rd = core.copy()                                # a good start, then a tail of mismatches: the read end lies below the best cell
    rf = follow.copy()
    rf[min(R, F) // 2:min(R, F)] = other[min(R, F) // 2:min(R, F)]
    add("good start, bad tail", rd, rf)
    rd2 = rd.copy()
    rd2[R // 2 + 3:] = ord("N")
    add("good start, trimmed", rd2, follow)
    if len(reads) % 2:
        add("follow", core, follow)
    return np.stack(reads), np.stack(refs), names


@pytest.mark.parametrize("G,K", [(8, 8), (16, 10)])
@pytest.mark.parametrize("R,F", [(12, 20), (33, 70), (40, 17)])
def test_planted_borders(R, F, G, K):
    reads, refs, names = _planted(R, F)
    Rp, Fp = ref.trimmed_lengths(reads), ref.trimmed_lengths(refs)
    at = {name: p for p, name in enumerate(names)}
    bonuses = (-1, 0, 4, ALWAYS)
    for form in FORMS:
        sc = _scoring(form)
        exp = ref.align(reads, refs, sc, _affine(form), end_bonus=bonuses, extended=True)
        best, always, mid = exp[0], exp[3], exp[2]
        texts = [[(op >> 4, op & 15) for op in o] for o in always[1]]
        # each planted case is there, by the reference alone
        for name in ("Rp 0 (NUL)", "Rp 0 (N)"):
            assert Rp[at[name]] == 0 and always[0][at[name]].tolist() == [0] * 6 and always[3][at[name]] is None
        for name in ("Fp 0", "Fp 0, short read"):
            p = at[name]
            assert Fp[p] == 0 and always[2][p, 4] == 0 and always[0][p, 3] == 0 and texts[p] == [(int(Rp[p]), ref.OP_I)] and exp[1][0][p, 3] == 0
            assert always[2][p, 3] < 0 and best[3][p] is None
        firsts = {name: ((best[1][at[name]] or [0])[0], (always[1][at[name]] or [0])[0]) for name in names if name.startswith("first")}
        for extra in (1, 3):            # (from the best cell: the read end of a read longer than the reference may move the gap)
            assert (extra << 4 | ref.OP_I) in firsts["first I %d" % extra] and (extra << 4 | ref.OP_D) in firsts["first D %d" % extra], firsts
        p = at["all mismatch"]
        assert best[2][p, 0] == 0 and best[3][p] is None and best[0][p].tolist() == [0] * 6 and always[2][p, 3] < 0 and always[0][p, 4] == always[2][p, 3]
        assert len(texts[at["homopolymer %d x %d" % (R, min(R, F) // 2)]]) >= 2
        # the two halves of a packed register: different Rp, Fp and different kinds of end under the bonus in between
        kinds = [None if e is None else ("read end" if e[0] + 1 == Rp[p] and mid[2][p, 3] + 4 >= mid[2][p, 0] else "best") for p, e in enumerate(mid[3])]
        assert any(kinds[p] != kinds[p + 1] and None not in kinds[p:p + 2] and Rp[p] != Rp[p + 1] and Fp[p] != Fp[p + 1] for p in range(0, len(kinds) - 1, 2)), kinds
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        for bonus, want in zip(bonuses, exp):
            _check(_run(eng, reads, refs, bonus, extended=True, stride=_stride(exp)), want, (R, F, G, K, form, bonus))
        # n odd and a partial wave
        for n in (1, 3, len(reads) - 1):
            _check(_run(eng, reads[:n], refs[:n], 4, extended=True, stride=_stride(exp)), tuple(part[:n] for part in mid), (R, F, G, K, form, "n", n))
        eng.close()


# ---- 5. ops_stride smaller than n_ops: the first ops are stored, n_ops is the whole count, nothing else is touched ----
def test_small_ops_stride():
    R, F, n = 33, 70, 40
    reads, refs = _batch(n, R, F, seed=5)
    sc = _scoring("aff")
    exp = ref.align(reads, refs, sc, True, end_bonus=ALWAYS, extended=True)
    assert max(len(o) for o in exp[1]) > 2 and min(len(o) for o in exp[1]) < 2
    eng = hipkernel.Engine(R, F, sc)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    recs = torch.full((n, 6), -7, dtype=torch.int32, device="cuda")
    ops = torch.full((n, 2), -7, dtype=torch.int32, device="cuda")
    ext = torch.full((n, 5), -7, dtype=torch.int32, device="cuda")
    eng.align_extend_device(0, d_reads, d_refs, end_bonus=ALWAYS, extended=True, ops_stride=2, out=(recs, ops, ext))
    torch.cuda.synchronize()
    eng.close()
    assert (recs.cpu().numpy().astype(np.int64) == exp[0]).all() and (ext.cpu().numpy().astype(np.int64) == exp[2]).all()
    got = ops.cpu().numpy()
    for p, want in enumerate(exp[1]):
        k = min(len(want), 2)
        assert got[p, :k].view(np.uint32).tolist() == want[:k] and (got[p, k:] == -7).all(), (p, got[p].tolist(), want)


# ---- 6. chunking: a call forced into several chunks equals one chunk ----
@pytest.mark.parametrize("by", ["rows", "pointers"])
def test_chunked_call_equals_one_chunk(monkeypatch, by):
    R, F, n = 33, 70, 12001
    reads, refs = _batch(n, R, F, seed=6)
    for form in ("lin", "aff"):
        sc = _scoring(form)
        eng = hipkernel.Engine(R, F, sc)
        whole = _run(eng, reads, refs, 6, stride=64)
        eng.close()
        if by == "rows":
            debug_switches(monkeypatch, cigar_rows_mb=1)            # 1 MiB / (2 x 104 bytes): 5 041 pairs, in whole blocks
        eng = hipkernel.Engine(R, F, sc)
        if by == "pointers":
            eng.set_pointer_scratch_cap_mb(1)
        _same(_run(eng, reads, refs, 6, stride=64), whole, (by, form))
        d = eng.describe(0, n)
        eng.close()
        debug_switches(monkeypatch, cigar_rows_mb=None)
        # the capped scratch stayed under its cap (and a margin of a tenth for the end cells and the rows' tail)
        held = d["cigar_rows_scratch_bytes"] if by == "rows" else d["extend_align_scratch_bytes"]
        assert 0 < held < 1.1 * (1 << 20), (by, held)
        _check(tuple(part[:96] for part in whole), tuple(part[:96] for part in ref.align(reads[:96], refs[:96], sc, _affine(form), end_bonus=6)), (by, form))


# ---- 7. the host entry equals the device entry, at 1 and 3 pipeline chunks, with and without extension records ----
@pytest.mark.parametrize("chunks", [1, 3])
def test_host_equals_device(monkeypatch, chunks):
    R, F, n = 33, 70, 3000
    if chunks == 3:
        debug_switches(monkeypatch, align_chunk_bytes=1000)         # (the pipeline's smallest chunk: 1 024 pairs)
    reads, refs = _batch(n, R, F, seed=7)
    for form in ("lin", "affsym"):
        eng = hipkernel.Engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs, 6, extended=True, stride=64)
        assert dev[0][:, 5].max() <= 64
        for with_extend in (True, False):
            for threads in (1, 4):
                recs, ops, offsets, ext = eng.align_extend_host(0, reads, refs, end_bonus=6, extended=True, with_extend=with_extend, threads=threads,
                                                                ops_cap=None if threads == 1 else 8)       # (8: too small, the call is repeated)
                names = hipkernel.aln_dtype().names
                assert (np.stack([recs[k] for k in names], axis=1).astype(np.int64) == dev[0]).all(), (form, with_extend, threads)
                assert offsets[0] == 0 and (np.diff(offsets) == dev[0][:, 5]).all() and len(ops) == offsets[n]
                for p in range(n):
                    assert (ops[offsets[p]:offsets[p + 1]] == dev[1][p, :dev[0][p, 5]]).all(), (form, p)
                if with_extend:
                    assert (np.stack([ext[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64) == dev[2]).all(), (form, threads)
                else:
                    assert ext is None
        recs, ops, offsets, ext = eng.align_extend_host(0, reads[:0], refs[:0])          # n = 0
        assert len(recs) == 0 and len(ops) == 0 and offsets.tolist() == [0]
        eng.close()


def _host_raw(eng, reads, refs, cap, ops_len, bonus, with_extend, threads=2):
    """valign_hip_align_extend_host as it stands: an ops buffer of ops_len entries and an ops_cap of `cap`, both marked"""
    n = len(reads)
    rp = (reads.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(reads.shape[1])).astype(np.uint64)
    fp = (refs.ctypes.data + np.arange(n, dtype=np.uint64) * np.uint64(refs.shape[1])).astype(np.uint64)
    recs = np.zeros(n, dtype=hipkernel.aln_dtype())
    ext = np.zeros(n, dtype=hipkernel.extend_dtype()) if with_extend else None
    ops = np.full(max(ops_len, 1), 0xDEADBEEF, np.uint32)
    offsets = np.full(n + 1, -7, np.int64)
    needed = ctypes.c_longlong(-7)
    rc = hipkernel.lib().valign_hip_align_extend_host(eng._h, 0, n, rp.ctypes.data, fp.ctypes.data, bonus, 1, recs.ctypes.data, ops.ctypes.data, cap,
                                                      offsets.ctypes.data, ctypes.byref(needed), ext.ctypes.data if with_extend else None, threads)
    return rc, recs, ops, offsets, needed.value, ext


@pytest.mark.parametrize("with_extend", [True, False])
def test_ops_cap_crossed_between_chunks(monkeypatch, with_extend):
    """Three chunks of 1 024, 1 024 and 452 pairs with ops_cap passed at a chunk border, one op before it and in the last chunk: the
    return code, the exact need, complete records, offsets and extension records, nothing written at or behind ops_cap, only the
    ops of the chunks that still fitted copied back, and the same engine serves the exact retry."""
    debug_switches(monkeypatch, align_chunk_bytes=4096)              # the floor: 1 024 pairs a chunk
    R, F, n = 33, 70, 2500
    reads, refs = _batch(n, R, F, seed=8)
    eng = hipkernel.Engine(R, F, _scoring("affsym"))
    recs, ops, offsets, ext = eng.align_extend_host(0, reads, refs, end_bonus=6, extended=True, with_extend=with_extend, threads=4)
    total, fixed = int(offsets[n]), (24 + (20 if with_extend else 0)) * n + 8 * 3
    d = eng.describe(0, n)
    assert d["ran_extend_align_chunks"] == 3 and d["cigar_d2h_bytes"] == fixed + 4 * total, d
    for cap, copied in ((int(offsets[1024]), int(offsets[1024])), (int(offsets[1024]) - 1, 0), (int(offsets[2048]), int(offsets[2048]))):
        assert 0 < cap < total
        rc, recs2, ops2, offsets2, needed, ext2 = _host_raw(eng, reads, refs, cap, total, 6, with_extend)
        assert rc != 0 and needed == total and "ops_cap" in hipkernel._err(), cap
        assert np.array_equal(recs2, recs) and np.array_equal(offsets2, offsets) and (ext2 is None if ext is None else np.array_equal(ext2, ext)), cap
        assert (ops2[cap:] == 0xDEADBEEF).all(), cap
        assert eng.describe(0, n)["cigar_d2h_bytes"] == fixed + 4 * copied, cap
        rc, recs3, ops3, offsets3, needed, ext3 = _host_raw(eng, reads, refs, total, total, 6, with_extend)
        assert rc == 0 and needed == total and np.array_equal(ops3, ops) and np.array_equal(offsets3, offsets) and np.array_equal(recs3, recs), cap
        assert ext3 is None if ext is None else np.array_equal(ext3, ext), cap
    eng.close()


# ---- 8. refusals ----
def test_refusals():
    R, F = 33, 70
    reads, refs = _batch(4, R, F, seed=3)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, word, opt=0, rd=d_reads, rf=d_refs, host=(reads, refs), **kw):
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.align_extend_device(opt, rd, rf, **kw)
        assert eng.describe(0, 4)["ran_extend_align"] == "none"
        kw.pop("ops_stride", None)
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.align_extend_host(opt, host[0], host[1], **kw)
        assert eng.describe(0, 4)["ran_extend_align"] == "none"

    sc = _scoring("lin")
    eng = hipkernel.Engine(R, F, sc)
    exp = ref.align(reads, refs, sc, False, end_bonus=3)
    _check(_run(eng, reads, refs, 3), exp, "before the refusals")
    assert eng.describe(0, 4)["ran_extend_align"] == "rows"
    refused(eng, "opt & 0xF == 0 only", opt=1)
    _check(_run(eng, reads, refs, 3), exp, "between the refusals")
    # opt & 0xF > 1 does nothing
    out = tuple(torch.full((4, w), -7, dtype=torch.int32, device="cuda") for w in (6, 8, 5))
    eng.align_extend_device(2, d_reads, d_refs, ops_stride=8, out=out)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == -7).all() for t in out)
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    for band_placed in (0, 1):
        eng.set_band_placed(band_placed)
        eng.set_band_width(16)
        refused(eng, "not built for band_width > 0")
        eng.set_band_width(0)
    eng.set_band_placed(0)
    eng.set_score_width(32)
    refused(eng, "score_width = 32")
    eng.set_extend_wide(1)
    refused(eng, "^extension alignments:")           # the extension scores of this call run on the int32 sweep
    assert eng.score_extend_device(0, d_reads, d_refs).shape == (4, 5) and eng.describe(0, 4)["ran_extend"] == "wide"
    eng.set_score_width(0)
    _check(_run(eng, reads, refs, 3), exp, "extend_wide = 1, a call the register sweep serves")
    eng.set_extend_wide(0)
    L = hipkernel.lib()
    bufs = [torch.empty(64, dtype=torch.int32, device="cuda").data_ptr() for _ in range(2)]
    assert L.valign_hip_align_extend_device(eng._h, 0, 4, d_reads.data_ptr(), d_refs.data_ptr(), -1, 2, bufs[0], bufs[1], 8, None, None) != 0
    assert b"extended must be 0" in L.valign_hip_last_error() and eng.describe(0, 4)["ran_extend_align"] == "none"
    with pytest.raises(hipkernel.HipKernelError, match="ops_stride must be >= 1"):
        eng.align_extend_device(0, d_reads, d_refs, ops_stride=0, out=(torch.empty((4, 6), dtype=torch.int32, device="cuda"),
                                                                       torch.empty((4, 0), dtype=torch.int32, device="cuda"), None))
    assert L.valign_hip_align_extend_device(eng._h, 0, 4, d_reads.data_ptr(), d_refs.data_ptr(), -1, 0, None, None, 8, None, None) != 0
    assert b"null result buffer" in L.valign_hip_last_error()
    needed = ctypes.c_longlong(0)
    assert L.valign_hip_align_extend_host(eng._h, 0, 4, None, None, -1, 0, None, None, 0, None, ctypes.byref(needed), None, 1) != 0
    assert b"null result buffer" in L.valign_hip_last_error()
    assert eng.describe(0, 4)["ran_extend_align"] == "none"
    _check(_run(eng, reads, refs, 3), exp, "after the refusals")
    eng.close()
    # cells that could leave int16: the top (33 x 970 > 32000) and the bottom (103 gap steps at -320); under extend_wide = 1 the
    # scores run wide, so the alignment's refusal is its own
    for scoring in (hipkernel.Scoring.make(970, -1, -3, -3), hipkernel.Scoring.make(2, -1, -320, -320)):
        eng = hipkernel.Engine(R, F, scoring)
        refused(eng, "signed int16 cells")
        eng.set_extend_wide(1)
        refused(eng, "^extension alignments:")
        eng.close()
    # the row strips: an unforced 1 500 x 1 500 call
    big = np.full((2, 1500), ord("A"), np.uint8)
    eng = hipkernel.Engine(1500, 1500, sc)
    refused(eng, "register sweep only", rd=torch.from_numpy(big).cuda(), rf=torch.from_numpy(big).cuda(), host=(big, big))
    eng.close()


# ---- 9. interleaving on one engine: the scratch the calls share ----
@pytest.mark.parametrize("form", ["lin", "aff"])
def test_interleaved_calls_equal_fresh_engines(form):
    R, F, n = 100, 260, 301
    reads, refs = _batch(n, R, F, seed=29)
    sc = _scoring(form)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def scores(eng):
        out = eng.score_extend_device(0, d_reads, d_refs)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def cigars(eng):
        recs, ops = eng.align_cigar_device(0, d_reads, d_refs, extended=True, ops_stride=48)
        torch.cuda.synchronize()
        recs, ops = recs.cpu().numpy(), ops.cpu().numpy()
        stored = np.arange(48)[None, :] < np.minimum(recs[:, 5], 48)[:, None]
        return recs, np.where(stored, ops, 0)

    fresh = []
    for call in (scores, cigars, lambda e: _run(e, reads, refs, 9, extended=True, stride=48), scores):
        eng = hipkernel.Engine(R, F, sc)
        fresh.append(call(eng))
        eng.close()
    eng = hipkernel.Engine(R, F, sc)
    assert (scores(eng) == fresh[0]).all()
    got = cigars(eng)
    assert (got[0] == fresh[1][0]).all() and (got[1] == fresh[1][1]).all()
    _same(_run(eng, reads, refs, 9, extended=True, stride=48), fresh[2], form)
    assert (scores(eng) == fresh[3]).all()
    got = cigars(eng)
    assert (got[0] == fresh[1][0]).all() and (got[1] == fresh[1][1]).all()
    eng.close()
    assert (fresh[2][2] == fresh[0]).all()          # the extension records of the alignment call are the score call's, bit for bit
    exp = ref.align(reads[:64], refs[:64], sc, _affine(form), end_bonus=9, extended=True)
    assert max(len(o) for o in exp[1]) > 48           # (some pairs overflow the stride: their first 48 ops are stored)
    _check(tuple(part[:64] for part in fresh[2]), (exp[0], [o[:48] for o in exp[1]], exp[2], exp[3]), form)
