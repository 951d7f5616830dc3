"""Banded extension alignments (key extend_band_align; align_extend_band_fill_kernel, extend_band_ends_kernel,
extend_band_walk_kernel) on the GPU: records, ops and extension records against tests/extend_band_align_ref.py with B = 8 (numpy /
Python, int64 cells, the whole matrix with absent cells, the walk on cell values; independent of the library).  Integers, compared
exactly, from the best cell (end_bonus -1), from the read end (INT32_MAX) and in between (20).

Every case first asserts its guards on the reference alone (_expect): some pair aligns; some banded record differs from the
unbanded one, except at the limit; at bonus 20 both kinds of end cell occur; and the properties its shape is meant to produce
occur -- an unreached read end, a walk that reaches the border column or the border row, a walk across a strip boundary, an end
cell in the last strip."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import extend_align_ref as ear
import extend_band_align_ref as ref
import extend_ref
from test_gpu_extend import FORMS, _affine, _scoring
from test_gpu_extend import _run as _run_scores
from test_gpu_extend_align import _run, _same
from test_gpu_extend_band import _band_batch as _scores_batch
from test_gpu_extend_band import _trim_reads
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

BASES = np.frombuffer(b"ACGT", np.uint8)
STRIP = 512
ALWAYS = ref.INT32_MAX
BONUSES = (-1, ALWAYS, 20)


def _band_batch(n, R, F, band_width, seed, short_ref=True):
    """the batch of the banded extension scores' tests without a literal '-' byte (the caveat of every CIGAR call: the encoder
    reads one as a gap): the interior junk byte of its references is '*'"""
    reads, refs = _scores_batch(n, R, F, band_width, seed, short_ref)
    refs[refs == ord("-")] = ord("*")
    return reads, refs


def _engine(R, F, sc, band_width, key=1, band=1, width=0, wide=0):
    eng = hipkernel.Engine(R, F, sc)
    eng.set_band_width(band_width)
    eng.set_extend_band(band)
    eng.set_extend_band_align(key)
    eng.set_score_width(width)
    eng.set_extend_wide(wide)
    return eng


def _ran_band(eng, n):
    d = eng.describe(0, n)
    assert d["ran_extend_align"] == "band" and d["ran_extend_align_geometry"] == "none" and d["extend_band_align"] == 1, d
    assert d["align_ptr_bytes_per_pair"] > 0 and d["extend_align_scratch_bytes"] > 0 and d["ran_extend_align_chunks"] >= 1, d
    return d


def _plant_short(reads, refs, p, L=20):
    """pair p: a read of L bases that the reference follows -- its read end is reached in every band, and chosen at bonus 20"""
    reads[p, L:] = ord("N")
    refs[p, :L] = reads[p, :L]


def _stride(exp):
    return max([len(o) for res in exp for o in res[1]] + [1]) + 2


def _expect(reads, refs, form, band_width, extended=False, match=2, mismatch=-1, limit=False, want=()):
    """-> scoring, the reference's results for BONUSES; the guards, on the reference alone"""
    sc, affine = _scoring(form, match, mismatch), _affine(form)
    R = reads.shape[1]
    exp = ref.align(reads, refs, sc, band_width, affine, end_bonus=BONUSES, extended=extended)
    free = extend_ref.extend(reads, refs, sc, affine=affine, chunk=16)
    best, always, mid = exp
    assert any(e is not None for e in best[3]), "no pair aligns"
    if limit:
        assert np.array_equal(best[2], free)
    else:
        assert (best[2] != free).any(), "the band changes no record"
    Rp = ref.trimmed_lengths(reads)
    kinds = {("read end" if mid[2][p, 3] + 20 >= mid[2][p, 0] else "best") for p, e in enumerate(mid[3]) if e is not None}
    assert kinds == {"read end", "best"}, kinds
    assert all(e is None or e[0] == Rp[p] - 1 for p, e in enumerate(always[3]) if always[2][p, 3] != ref.UNREACHED)
    moves = [m for res in exp for path in res[4] for m in path]
    has = {"unreached": (best[2][:, 3] == ref.UNREACHED).any(),
           "border_col": any(j == -1 for _, _, j in moves),
           "border_row": any(i == -1 for _, i, _j in moves),
           "cross": any(len({i // STRIP for _, i, _j in path if i >= 0}) > 1 for res in exp for path in res[4]),
           "last_strip": any(e is not None and e[0] // STRIP == (R - 1) // STRIP for res in exp for e in res[3])}
    for prop in want:
        assert has[prop], prop
    return sc, exp


def _check(got, exp, what):
    recs, ops, ext = got
    exp_recs, exp_ops, exp_ext = exp[:3]
    bad = np.nonzero((recs != exp_recs).any(axis=1))[0]
    assert bad.size == 0, (what, "records of pairs", bad[:8].tolist(), "got", recs[bad[:4]].tolist(), "expected", exp_recs[bad[:4]].tolist())
    for p, want in enumerate(exp_ops):
        assert ops[p, :len(want)].tolist() == want, (what, "ops of pair", p, ops[p, :len(want)].tolist()[:12], want[:12])
    if ext is not None:
        bad = np.nonzero((ext != exp_ext).any(axis=1))[0]
        assert bad.size == 0, (what, "extension records of pairs", bad[:8].tolist(), ext[bad[:4]].tolist(), exp_ext[bad[:4]].tolist())


def _all_bonuses(eng, reads, refs, exp, what, extended=False):
    for bonus, want in zip(BONUSES, exp):
        _check(_run(eng, reads, refs, bonus, extended=extended, stride=_stride(exp)), want, what + (bonus,))


# ---- 1. one strip: 33 x 70, five pairs (the last wave holds one) and one pair, bands from w = 0 to the unbanded limit ----
@pytest.mark.parametrize("band_width", [1, 2, 9, 17, 40, 400])
@pytest.mark.parametrize("form", list(FORMS))
def test_one_strip(form, band_width):
    R, F = 33, 70
    reads, refs = _band_batch(5, R, F, band_width, seed=41 + band_width)
    limit = band_width // 2 >= max(R, F)
    sc, exp = _expect(reads, refs, form, band_width, extended=True, limit=limit, want=() if limit else ("unreached",))
    eng = _engine(R, F, sc, band_width)
    for n in (5, 1):
        _all_bonuses(eng, reads[:n], refs[:n], [tuple(part[:n] for part in res) for res in exp], (form, band_width, n), extended=True)
        _ran_band(eng, n)
    # the extension records are banded extension scores', on the same engine
    scores = _run_scores(eng, reads, refs)
    assert np.array_equal(scores, exp[0][2]) and eng.describe(0, 5)["ran_extend"] == "band"
    eng.close()
    if limit:           # the register sweep serves this call: its result
        other = hipkernel.Engine(R, F, sc)
        for bonus, want in zip(BONUSES, exp):
            got = _run(other, reads, refs, bonus, extended=True, stride=_stride(exp))
            assert other.describe(0, 5)["ran_extend_align"] == "rows"
            _check(got, want, (form, "the register sweep", bonus))
        other.close()
        unbanded = ear.align(reads, refs, sc, _affine(form), end_bonus=BONUSES, extended=True)
        for res, want in zip(exp, unbanded):
            assert np.array_equal(res[0], want[0]) and res[1] == want[1]


# ---- 2. the last pointer block with lane 63 active: 127, 128 and 129 steps (a block of 7, a whole one, a block of 1) ----
@pytest.mark.parametrize("F", [64, 65, 66])
@pytest.mark.parametrize("R", [505, 512])
def test_last_pointer_block(R, F):
    band_width = 1200
    assert F + 63 == {64: 127, 65: 128, 66: 129}[F] and (R - 1) // 8 == 63
    reads, refs = _band_batch(6, R, F, band_width, seed=R + F)
    for p in (0, 3):            # the reference is the read's tail: the read end's best candidate is the last column
        refs[p] = reads[p, R - F:]
    _plant_short(reads, refs, 5, 40)
    for form in ("lin", "aff"):
        sc, exp = _expect(reads, refs, form, band_width, limit=True, want=("border_col",))
        assert any(e is not None and e == (R - 1, F - 1) for e in exp[1][3]), "no read-end walk starts in column F - 1"
        eng = _engine(R, F, sc, band_width)
        _all_bonuses(eng, reads, refs, exp, (R, F, form))
        _ran_band(eng, 6)
        eng.close()


# ---- 3. two strips: window offsets at the 64-column blocks, an empty second strip (F <= 129), row Rp - 1 in either strip,
# unreached read ends ----
@pytest.mark.parametrize("band_width", [2, 16, 127, 128, 130])
@pytest.mark.parametrize("F", [63, 64, 65, 129, 600])
@pytest.mark.parametrize("R", [513, 520])
def test_two_strips(R, F, band_width):
    lengths = [100, 512, 513, R]
    reads, refs = _band_batch(10, R, F, band_width, seed=R + F + band_width, short_ref=F > 129)
    reads = _trim_reads(reads, lengths, pairs=[4, 5, 7, 8])
    _plant_short(reads, refs, 9)
    Rp = ref.trimmed_lengths(reads)
    assert set(lengths) <= set(Rp.tolist()) and (Rp <= STRIP).any() and (Rp > STRIP).any()
    for form in ("lin", "aff"):
        sc, exp = _expect(reads, refs, form, band_width, want=("unreached",) + (("cross", "last_strip") if F == 600 else ()))
        eng = _engine(R, F, sc, band_width)
        _all_bonuses(eng, reads, refs, exp, (R, F, band_width, form))
        _ran_band(eng, 10)
        eng.close()


# ---- 4. gaps planted over the strip boundary: a vertical run over rows 508 .. 516 (the F boundary row, the gap bit of row 512),
# a horizontal run in row 511 and one in row 512 ----
def _runs(path, kind):
    """maximal runs of `kind` moves -> a list of (rows, columns) of each run"""
    runs, cur = [], None
    for k, i, j in path:
        if k == kind:
            cur = cur or ([], [])
            cur[0].append(i)
            cur[1].append(j)
        elif cur:
            runs.append(cur)
            cur = None
    if cur:
        runs.append(cur)
    return runs


def test_gaps_over_the_strip_boundary():
    R, F, band_width = 520, 600, 40
    reads, refs = _band_batch(8, R, F, band_width, seed=4)
    rng = np.random.default_rng(44)
    # the planted bases are A's, and neither sequence holds another A from position 490 on: the A's match nothing they could
    # reach, so each run lies exactly where it was planted (mismatch -9: a gap is cheaper than mismatching through it)
    for p in (0, 1, 3):
        reads[p] = BASES[rng.integers(0, 4, R)]
        reads[p, 490:][reads[p, 490:] == ord("A")] = ord("C")
        refs[p] = BASES[rng.integers(1, 4, F)]
    reads[0, 508:517] = ord("A")                                                            # read bases 508 .. 516 face a gap
    refs[0, :R - 9] = np.concatenate([reads[0, :508], reads[0, 517:]])
    for p, row in ((1, 511), (3, 512)):                                                     # five reference bases behind read base `row`
        refs[p, :R + 5] = np.concatenate([reads[p, :row + 1], np.full(5, ord("A"), np.uint8), reads[p, row + 1:]])
    _plant_short(reads, refs, 5)
    for form in ("lin", "aff"):
        sc, exp = _expect(reads, refs, form, band_width, mismatch=-9, want=("cross", "last_strip"))
        paths = exp[1][4]               # from the read end
        assert [rows for rows, _ in _runs(paths[0], "I")] == [list(range(508, 517))], _runs(paths[0], "I")
        for p, row in ((1, 511), (3, 512)):
            assert [rows for rows, _ in _runs(paths[p], "D")] == [[row] * 5], (p, _runs(paths[p], "D"))
        eng = _engine(R, F, sc, band_width)
        _all_bonuses(eng, reads, refs, exp, (form,))
        eng.close()


# ---- 5. three strips: both ping-pong slots reused, an end cell in the third strip ----
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_three_strips(form):
    R, F, band_width = 1030, 1100, 64
    reads, refs = _band_batch(6, R, F, band_width, seed=5)
    _plant_short(reads, refs, 5)
    sc, exp = _expect(reads, refs, form, band_width, want=("unreached", "cross", "last_strip"))
    assert (R - 1) // STRIP == 2
    eng = _engine(R, F, sc, band_width)
    _all_bonuses(eng, reads, refs, exp, (form,))
    _ran_band(eng, 6)
    eng.close()


# ---- 6. halves and waves: two pairs of one wave with very different Rp / Fp, an odd last wave, the batch reversed ----
def test_halves_and_waves():
    R, F, band_width = 520, 600, 40
    rng = np.random.default_rng(6)
    reads = BASES[rng.integers(0, 4, (5, R))]
    refs = BASES[rng.integers(0, 4, (5, F))]
    for p, (Rp, Fp) in enumerate([(520, 600), (30, 50), (100, 600), (520, 40), (517, 530)]):
        refs[p, :min(Rp, Fp)] = reads[p, :min(Rp, Fp)]
        reads[p, Rp:] = ord("N")
        refs[p, Fp:] = 0
    refs[4, 300:530] = refs[4, 297:527].copy()              # three bases more in the reference, inside the band
    assert ref.trimmed_lengths(reads).tolist() == [520, 30, 100, 520, 517] and ref.trimmed_lengths(refs).tolist() == [600, 50, 600, 40, 530]
    for form in ("lin", "aff"):
        sc, exp = _expect(reads, refs, form, band_width, want=("unreached", "cross", "last_strip"))
        eng = _engine(R, F, sc, band_width)
        _all_bonuses(eng, reads, refs, exp, (form,))
        back = [tuple(part[::-1] for part in res) for res in exp]
        _all_bonuses(eng, np.ascontiguousarray(reads[::-1]), np.ascontiguousarray(refs[::-1]), back, (form, "reversed"))
        for n in (1, 3):
            _check(_run(eng, reads[:n], refs[:n], 20, stride=_stride(exp)), tuple(part[:n] for part in exp[2]), (form, "n", n))
        eng.close()


# ---- 7. chunks and overflow ----
@functools.lru_cache(maxsize=None)
def _nine():
    R, F, band_width = 520, 600, 40
    reads, refs = _band_batch(9, R, F, band_width, seed=7)
    _plant_short(reads, refs, 5)
    sc, exp = _expect(reads, refs, "aff", band_width, want=("cross",))
    return reads, refs, sc, exp


@pytest.mark.parametrize("band_width", [40, 1200])
def test_chunks(band_width):
    R, F = 520, 600
    reads, refs, sc, exp = _nine()
    if band_width != 40:
        _, exp = _expect(reads, refs, "aff", band_width, limit=True)
    eng = _engine(R, F, sc, band_width)
    whole = _run(eng, reads, refs, 20, stride=_stride(exp))
    per_pair = _ran_band(eng, 9)["align_ptr_bytes_per_pair"]
    eng.close()
    _check(whole, exp[2], ("one chunk", band_width))
    assert 2 * per_pair <= (1 << 20) < 6 * per_pair                 # a MiB holds the pointers of one or two waves, not of three
    eng = _engine(R, F, sc, band_width)
    eng.set_pointer_scratch_cap_mb(1)
    got = _run(eng, reads, refs, 20, stride=_stride(exp))
    d = _ran_band(eng, 9)
    eng.close()
    assert d["ran_extend_align_chunks"] >= 3, d["ran_extend_align_chunks"]
    _same(got, whole, ("chunked", band_width))


def test_small_ops_stride():
    R, F, band_width = 520, 600, 40
    reads, refs, sc, exp = _nine()
    want = exp[1]
    longest = max(len(o) for o in want[1])
    assert longest > 3
    eng = _engine(R, F, sc, band_width)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    for stride in (1, longest - 1):
        recs = torch.full((9, 6), -7, dtype=torch.int32, device="cuda")
        ops = torch.full((9, stride), -7, dtype=torch.int32, device="cuda")
        ext = torch.full((9, 5), -7, dtype=torch.int32, device="cuda")
        eng.align_extend_device(0, d_reads, d_refs, end_bonus=ALWAYS, ops_stride=stride, out=(recs, ops, ext))
        torch.cuda.synchronize()
        assert (recs.cpu().numpy().astype(np.int64) == want[0]).all() and (ext.cpu().numpy().astype(np.int64) == want[2]).all()
        got = ops.cpu().numpy()
        for p, pair_ops in enumerate(want[1]):
            k = min(len(pair_ops), stride)
            assert got[p, :k].view(np.uint32).tolist() == pair_ops[:k] and (got[p, k:] == -7).all(), (stride, p)
    eng.close()


# ---- 8. the host entry: threads 1 and 3 equal the device entry; an ops_cap that is too small ----
def test_host_entry():
    R, F, band_width = 520, 600, 40
    reads, refs, sc, exp = _nine()
    eng = _engine(R, F, sc, band_width)
    dev = _run(eng, reads, refs, 20, extended=False, stride=_stride(exp))
    _check(dev, exp[2], "device")
    names = hipkernel.aln_dtype().names
    for threads in (1, 3):
        recs, ops, offsets, ext = eng.align_extend_host(0, reads, refs, end_bonus=20, threads=threads)
        assert eng.describe(0, 9)["ran_extend_align"] == "band"
        assert (np.stack([recs[k] for k in names], axis=1).astype(np.int64) == dev[0]).all(), threads
        assert offsets[0] == 0 and (np.diff(offsets) == dev[0][:, 5]).all() and len(ops) == offsets[9]
        for p in range(9):
            assert (ops[offsets[p]:offsets[p + 1]] == dev[1][p, :dev[0][p, 5]]).all(), (threads, p)
        assert (np.stack([ext[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64) == dev[2]).all(), threads
    # ops_cap too small: non-zero, ops_needed reported, the records complete
    total = int(dev[0][:, 5].sum())
    assert total > 2
    L = hipkernel.lib()
    rp = (reads.ctypes.data + np.arange(9, dtype=np.uint64) * np.uint64(R)).astype(np.uint64)
    fp = (refs.ctypes.data + np.arange(9, dtype=np.uint64) * np.uint64(F)).astype(np.uint64)
    recs = np.zeros(9, dtype=hipkernel.aln_dtype())
    ops = np.zeros(2, dtype=np.uint32)
    offsets = np.zeros(10, dtype=np.int64)
    needed = ctypes.c_longlong(0)
    rc = L.valign_hip_align_extend_host(eng._h, 0, 9, rp.ctypes.data, fp.ctypes.data, 20, 0, recs.ctypes.data, ops.ctypes.data, 2, offsets.ctypes.data,
                                        ctypes.byref(needed), None, 1)
    assert rc != 0 and needed.value == total
    assert (np.stack([recs[k] for k in names], axis=1).astype(np.int64) == dev[0]).all()
    eng.close()


# ---- 9. beyond int16: 33 x 70 at match 1000 (33 000 > 32 000); the register route refuses this call ----
@pytest.mark.parametrize("band_width", [17, 400])
def test_beyond_int16(band_width):
    R, F = 33, 70
    reads, refs = _band_batch(5, R, F, band_width, seed=9)
    limit = band_width == 400
    for form in ("lin", "aff"):
        sc, exp = _expect(reads, refs, form, band_width, match=1000, limit=limit)
        assert exp[0][0][:, 4].max() > 32767
        plain = hipkernel.Engine(R, F, sc)
        with pytest.raises(hipkernel.HipKernelError, match="signed int16 cells"):
            plain.align_extend_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        plain.close()
        eng = _engine(R, F, sc, band_width)
        _all_bonuses(eng, reads, refs, exp, (form, band_width))
        eng.close()
        if limit:
            unbanded = ear.align(reads, refs, sc, _affine(form), end_bonus=BONUSES)
            for res, want in zip(exp, unbanded):
                assert np.array_equal(res[0], want[0]) and res[1] == want[1]


# ---- 10. the key and the refusals ----
def test_key_and_refusals():
    R, F, band_width = 33, 70, 17
    reads, refs = _band_batch(5, R, F, band_width, seed=10)
    sc, exp = _expect(reads, refs, "lin", band_width)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, word, opt=0, rd=d_reads, rf=d_refs, host=(reads, refs)):
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.align_extend_device(opt, rd, rf)
        assert eng.describe(0, 5)["ran_extend_align"] == "none"
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.align_extend_host(opt, host[0], host[1])
        assert eng.describe(0, 5)["ran_extend_align"] == "none"

    eng = _engine(R, F, sc, band_width, key=0)
    refused(eng, "^extension alignments: not built under a band")                # key off: the two texts of today
    eng.set_extend_band(0)
    refused(eng, "^extension scores are not built for band_width > 0")
    eng.set_extend_band_align(1)
    refused(eng, "^extension scores are not built for band_width > 0")         # key on without extend_band: the band text
    eng.set_band_width(0)                                                        # no band: the register sweep, results unchanged
    unbanded = ear.align(reads, refs, sc, False, end_bonus=20)
    got = _run(eng, reads, refs, 20, stride=_stride(exp))
    assert eng.describe(0, 5)["ran_extend_align"] == "rows"
    _check(got, unbanded, "no band")
    with pytest.raises(hipkernel.HipKernelError, match="extend_band_align must be 0 or 1"):
        eng.set_extend_band_align(2)
    assert eng.describe(0, 5)["extend_band_align"] == 1
    eng.set_band_width(band_width)
    eng.set_extend_band(1)
    _check(_run(eng, reads, refs, 20, stride=_stride(exp)), exp[2], "the key on")
    eng.set_score_width(16)
    refused(eng, "^extend_band:.*score_width = 16")
    eng.set_score_width(0)
    refused(eng, "opt & 0xF == 0 only", opt=1)
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    # opt & 0xF > 1 does nothing
    out = tuple(torch.full((5, w), -7, dtype=torch.int32, device="cuda") for w in (6, 8, 5))
    eng.align_extend_device(2, d_reads, d_refs, ops_stride=8, out=out)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy() == -7).all() for t in out)
    L = hipkernel.lib()
    bufs = [torch.empty(64, dtype=torch.int32, device="cuda").data_ptr() for _ in range(2)]
    assert L.valign_hip_align_extend_device(eng._h, 0, 5, d_reads.data_ptr(), d_refs.data_ptr(), -1, 2, bufs[0], bufs[1], 8, None, None) != 0
    assert b"extended must be 0" in L.valign_hip_last_error() and eng.describe(0, 5)["ran_extend_align"] == "none"
    assert L.valign_hip_align_extend_device(eng._h, 0, 5, d_reads.data_ptr(), d_refs.data_ptr(), -1, 0, bufs[0], bufs[1], 0, None, None) != 0
    assert b"ops_stride must be >= 1" in L.valign_hip_last_error()
    assert L.valign_hip_align_extend_device(eng._h, 0, 5, d_reads.data_ptr(), d_refs.data_ptr(), -1, 0, None, None, 8, None, None) != 0
    assert b"null result buffer" in L.valign_hip_last_error()
    _all_bonuses(eng, reads, refs, exp, ("after the refusals",))               # the engine still answers
    eng.close()
    # the band's int32 range: 10 000 gap steps at -30 000 (the refusal comes before anything is launched)
    big = np.full((2, 5000), ord("A"), np.uint8)
    eng = _engine(5000, 5000, hipkernel.Scoring.make(2, -1, -30000, -30000), 64)
    refused(eng, "^extend_band: shape x scoring", rd=torch.from_numpy(big).cuda(), rf=torch.from_numpy(big).cuda(), host=(big, big))
    eng.close()


def test_one_engine_alternates_calls():
    """banded extension scores, banded extension alignments, unbanded align_cigar_device (the shared pointer scratch) and banded
    extension alignments again: every result equals a fresh engine's"""
    R, F, band_width = 520, 600, 40
    reads, refs, sc, exp = _nine()
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def cigar(eng):
        eng.set_band_width(0)
        recs, ops = eng.align_cigar_device(0, d_reads, d_refs, ops_stride=64)
        torch.cuda.synchronize()
        eng.set_band_width(band_width)
        return recs.cpu().numpy(), ops.cpu().numpy()

    fresh = []
    for step in range(3):
        eng = _engine(R, F, sc, band_width)
        fresh.append([lambda e: _run_scores(e, reads, refs), lambda e: _run(e, reads, refs, 20, stride=_stride(exp)), cigar][step](eng))
        eng.close()
    assert np.array_equal(fresh[0], exp[2][2])
    _check(fresh[1], exp[2], "a fresh engine")
    eng = _engine(R, F, sc, band_width)
    assert np.array_equal(_run_scores(eng, reads, refs), fresh[0])
    _same(_run(eng, reads, refs, 20, stride=_stride(exp)), fresh[1], "after the scores")
    recs, ops = cigar(eng)
    stored = np.arange(64)[None, :] < np.minimum(recs[:, 5], 64)[:, None]
    assert np.array_equal(recs, fresh[2][0]) and np.array_equal(ops[stored], fresh[2][1][stored])
    _same(_run(eng, reads, refs, 20, stride=_stride(exp)), fresh[1], "after the unbanded alignment")
    assert np.array_equal(_run_scores(eng, reads, refs), fresh[0])
    eng.close()
