"""Suboptimal Smith-Waterman scores on the GPU (valign_hip_score_subopt_device / _host): the placed record plus the runner-up
score and its column from the one placed sweep, against tests/subopt_ref.py (numpy, int64 cells, the whole matrix, independent
of the library).  Integers, compared exactly."""
import numpy as np
import pytest
import torch

import instance_matrix as im
import subopt_cases as cases
import subopt_ref
from conftest import debug_switches
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]
# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _affine(form):
    return len(FORMS[form]) > 2


def _run(eng, reads, refs, mask, opt=0, stream=None):
    out = eng.score_subopt_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), mask, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _host(eng, reads, refs, mask, threads=1):
    got = eng.score_subopt_host(0, reads, refs, mask, threads=threads)
    assert got.dtype == hipkernel.subopt_dtype() and got.shape == (len(reads),)
    return np.stack([got[k] for k in hipkernel.subopt_dtype().names], axis=1).astype(np.int64)


def _check(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


def _bits(K):
    return 2 if K <= 4 else (3 if K <= 8 else 4)


def _rows_match(R, F, K):
    """the smallest match score beyond the lane key's range (placed_choice: (min(R, F) match + 1) << bits > 32000)"""
    m = 32000 // (min(R, F) << _bits(K)) + 1
    assert ((min(R, F) * m + 1) << _bits(K)) > 32000 and min(R, F) * m + 1 <= 32000
    return m


def _trim_half(reads, rng):
    for p in range(0, len(reads), 2):
        reads[p, rng.integers(1, reads.shape[1] + 1):] = rng.choice([0, ord("N")])
    return reads


# ---- 1. every compiled instance: six full geometries x both tracks x four gap forms, at the instance matrix's shapes ----
@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("G,K", FULL)
def test_every_instance(G, K, shape):
    rng = np.random.default_rng(G * K + shape)
    n = im.batch(G)
    R, F = im.shapes(G, K)[shape]
    ran = set()
    reads, refs, _ = cases.fuzz_batch(n, R, F, seed=R + F, plant_at=min(2, F - 1))
    reads = _trim_half(reads, rng)
    for track in (("key", "rows") if K <= 16 else ("rows",)):
        match = 2 if track == "key" else _rows_match(R, F, K)
        for form in FORMS:
            sc = _scoring(form, match, -1 if track == "key" else -(match // 2))
            prep = subopt_ref.prepare(reads, refs, sc, affine=_affine(form), chunk=64)
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            for mask in (0, G, F):
                got = _run(eng, reads, refs, mask)
                _check(got, subopt_ref.apply_mask(prep, mask), (G, K, R, F, track, form, mask))
            d = eng.describe(0, n)
            eng.close()
            assert d["ran_subopt"] == track and d["subopt_ring_cols"] == 4 * G, (G, K, R, F, track, form, d["ran_subopt"])
            assert d["ran_subopt_geometry"] == "%dx%d" % (G, K), (G, K, R, F, track, form, d["ran_subopt_geometry"])
            ran.add((track, form))
    assert len(ran) == (8 if K <= 16 else 4)


# ---- 2. ring and sweep edges ----
def test_ring_and_sweep_edges():
    R, G = 150, 16
    sc = _scoring("sym")
    eng = hipkernel.Engine(R, 1, sc, group_lanes=16, rows_per_lane=10)
    _run(eng, *cases.fuzz_batch(9, R, 1, seed=1, plant_at=0)[:2], 0)
    ring = eng.describe(0, 9)["subopt_ring_cols"]
    eng.close()
    assert ring == 64
    for F in (1, 2, G - 1, G, ring - 1, ring, ring + 1, 2 * ring + 3):
        reads, refs, _ = cases.fuzz_batch(9, R, F, seed=F, plant_at=0)
        refs[:, :F] = reads[:, 10:10 + F]                    # every column scores: column maxima grow up to the last one
        refs[4:, F // 2] ^= 6                                # ... and a mismatch in the middle for half of them
        for form in ("sym", "aff"):
            sc = _scoring(form)
            prep = subopt_ref.prepare(reads, refs, sc, affine=_affine(form))
            eng = hipkernel.Engine(R, F, sc, group_lanes=16, rows_per_lane=10)
            for mask in (0, 3, F):
                _check(_run(eng, reads, refs, mask), subopt_ref.apply_mask(prep, mask), (F, form, mask))
            eng.close()


# ---- 3. window edges ----
# A second copy is planted only where it lies BESIDE the best copy (its end at least L + 2 columns from the best end).  A copy
# that ends nearer overlaps the best copy in the reference, so it cannot be planted whole, and what the candidates hold there is
# the best alignment's own prefixes and extensions, which outscore it.  So at masks 0, 1 and F no second copy exists: masks 0 and
# 1 check the edge on those prefixes (column mask + 1 from the end counts, with its stated value; column mask does not), mask F
# checks that nothing counts, and mask 30 -- added to the masks of the definition's list for this purpose -- checks a planted
# copy excluded at distance mask and counted at mask + 1, on each side of each of the three positions where it fits.
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_window_edges(form):
    R, F, L = 24, 150, 24
    sc = _scoring(form)
    rd = np.frombuffer(b"ACGACCGAGCAGGCACGAGCCAGC", np.uint8)
    second = cases.mutate(rd, [6, 12, 18])
    for mask in (0, 1, 30, F):
        reads, refs, counted = [], [], []
        for best_at in (0, 60, F - L):                        # the best copy ends in column L - 1, in the middle, in the last column
            best_end = best_at + L - 1
            for side in (-1, 1):
                for dist in (mask, mask + 1):                 # the second copy's end: excluded at distance mask, counted one further
                    end2 = best_end + side * dist
                    ref = np.full(F, ord("T"), np.uint8)
                    fits = L - 1 <= end2 < F and dist >= L + 2            # beside the best copy (closer, the best alignment's own partial scores are the candidates)
                    if fits:
                        ref[end2 - L + 1:end2 + 1] = second
                    ref[best_at:best_at + L] = rd
                    reads.append(rd)
                    refs.append(ref)
                    counted.append(end2 + 1 if fits and dist > mask else 0)
        reads, refs, counted = np.array(reads), np.array(refs), np.array(counted)
        exp = subopt_ref.subopt(reads, refs, sc, mask, affine=_affine(form))
        assert (exp[:, 0] == 48).all()
        assert ((np.abs(exp[:, 4] - exp[:, 2]) > mask) | (exp[:, 3] == 0)).all()
        assert (exp[counted > 0, 3] == 39).all() and (exp[counted > 0, 4] == counted[counted > 0]).all()
        if mask >= L:
            assert (exp[counted == 0, 3] < 39).all()          # at distance mask the second copy's end is not counted
        if mask == F:
            assert (exp[:, 3:] == 0).all()
        if mask == 30:
            assert (counted > 0).sum() == 4 and (exp[:, 4] < exp[:, 2]).any() and (exp[:, 4] > exp[:, 2]).any()
        if mask < 2:
            assert (exp[:, 3] == 48 - 2 * (mask + 1)).all()   # the best alignment's own prefix, one column outside the window
        for G, K in ((0, 0), (8, 8)):
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            _check(_run(eng, reads, refs, mask), exp, (form, mask, G, K))
            eng.close()
    # a second copy with three mismatches, one column outside / inside the window, stated by hand (linear and affine alike)
    ref = np.full((2, F), ord("T"), np.uint8)
    ref[:, 20:44] = rd
    ref[:, 90:114] = second
    eng = hipkernel.Engine(R, F, sc)
    got = _run(eng, np.array([rd, rd]), ref, 113 - 43 - 1)
    assert got.tolist() == [[48, 24, 44, 39, 114]] * 2
    got = _run(eng, np.array([rd, rd]), ref, 113 - 43)
    eng.close()
    assert (got[:, :3] == [48, 24, 44]).all() and (got[:, 3] < 39).all()


# ---- 4. ties ----
@pytest.mark.parametrize("G,K", [(0, 0), (16, 10), (64, 8)])
def test_ties(G, K):
    R, F = 8, 80
    rd = np.frombuffer(b"ACGACCGA", np.uint8)
    refs = np.full((4, F), ord("T"), np.uint8)
    refs[0, 40:48] = rd
    refs[0, 10:15] = rd[:5]
    refs[0, 65:70] = rd[:5]                 # equal runner-ups left and right of the window: the smaller column
    refs[1, 10:18] = rd
    refs[1, 50:58] = rd                     # two exact copies: score2 == score at the later column
    refs[2, 40:48] = rd
    refs[2, 65:70] = rd[:5]
    refs[2, 72:77] = rd[:5]                 # both on the right
    refs[3, 0:8] = rd
    refs[3, 72:80] = rd                     # first and last possible column
    reads = np.tile(rd, (4, 1))
    for form in ("sym", "aff"):
        sc = _scoring(form)
        exp = subopt_ref.subopt(reads, refs, sc, 6, affine=_affine(form))
        assert exp[:3].tolist() == [[16, 8, 48, 10, 15], [16, 8, 18, 16, 58], [16, 8, 48, 10, 70]] and exp[3].tolist() == [16, 8, 8, 16, 80]
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        _check(_run(eng, reads, refs, 6), exp, (G, K, form))
        eng.close()


# ---- 5. ragged batches ----
def test_ragged_batches():
    R, F = 150, 500
    rng = np.random.default_rng(17)
    n = 40
    reads, refs, _ = cases.fuzz_batch(n, R, F, seed=2, plant_at=30)
    refs[:, 300:300 + 100] = np.array([cases.mutate(reads[p, :100], [20, 50, 80]) for p in range(n)])
    for p in range(n):                      # the two pairs of a register differ in both trimmed lengths
        if p % 4 != 3:
            reads[p, rng.integers(20, R):] = (0, ord("N"))[p % 2]
            refs[p, rng.integers(200, F):] = (0, ord("N"))[(p // 2) % 2]
    reads[5] = ord("N")                     # an all-N read
    refs[6] = ord("N")                      # an all-N reference
    refs[8:16, 50:] = 0                     # a wave of 16 x 10 whose references all end early
    refs[16:24, 0:] = 0                     # ... and one without any reference base
    for form in ("sym", "aff"):
        sc = _scoring(form)
        prep = subopt_ref.prepare(reads, refs, sc, affine=_affine(form), chunk=64)
        for G, K in ((16, 10), (0, 0)):
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            for mask in (0, 75, 20):
                exp = subopt_ref.apply_mask(prep, mask)
                _check(_run(eng, reads, refs, mask), exp, (form, G, K, mask))
            eng.close()
        assert (exp[[5, 6] + list(range(16, 24))] == 0).all() and (exp[[0, 1, 2, 4], 3] > 0).all()


def test_padded_reads_do_not_repeat_their_score():
    R, F, mask = 40, 120, 15
    for pad in (0, ord("N")):
        batches = [cases.planted(4, R, F, seed=L, read_len=L, at=50, pad=pad) for L in (30, 20, 12)]
        reads = np.concatenate([b[0] for b in batches])
        refs = np.concatenate([b[1] for b in batches])
        for form, (G, K) in (("sym", (0, 0)), ("aff", (8, 8)), ("lin", (16, 10))):
            sc = _scoring(form)
            exp = subopt_ref.subopt(reads, refs, sc, mask, affine=_affine(form))
            assert exp[:, 0].tolist() == [60] * 4 + [40] * 4 + [24] * 4
            all_rows = subopt_ref.subopt(reads, refs, sc, mask, affine=_affine(form), trim=False)
            assert (all_rows[4:, 3] == all_rows[4:, 0]).all()                  # through the padding the best score leaves the window
            eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
            got = _run(eng, reads, refs, mask)
            eng.close()
            _check(got, exp, (pad, form))
            assert (got[:, 3] < got[:, 0]).all()


# ---- 6. call shape ----
def test_batch_sizes():
    R, F = 150, 500
    reads, refs, _ = cases.fuzz_batch(70, R, F, seed=3, plant_at=100)
    sc = _scoring("sym")
    exp = subopt_ref.subopt(reads, refs, sc, 75, chunk=70)
    eng = hipkernel.Engine(R, F, sc)
    d = eng.describe(0, 70)
    ppb = d["pairs_per_wave"] * d["waves_per_block"]
    assert ppb + 1 <= 70
    for n in (1, 2, ppb - 1, ppb, ppb + 1, 70):
        _check(_run(eng, reads[:n], refs[:n], 75), exp[:n], n)
    eng.close()


def test_a_call_of_four_chunks_equals_one_chunk(monkeypatch):
    R, F = 150, 500
    n = 56
    reads, refs, _ = cases.fuzz_batch(n, R, F, seed=4, plant_at=60)
    sc = _scoring("aff")
    exp = subopt_ref.subopt(reads, refs, sc, 75, affine=True, chunk=n)
    eng = hipkernel.Engine(R, F, sc)
    one = _run(eng, reads, refs, 75)
    d = eng.describe(0, n)
    eng.close()
    ppw = d["pairs_per_wave"]
    assert ppw == 8 and d["subopt_scratch_bytes"] >= n // 2 * F * 4
    debug_switches(monkeypatch, subopt_scratch_bytes=(2 * ppw // 2) * F * 4)       # 16 pairs a chunk: four chunks, the last one of 8
    eng = hipkernel.Engine(R, F, sc)
    cut = _run(eng, reads, refs, 75)
    held = eng.describe(0, n)["subopt_scratch_bytes"]
    eng.close()
    assert 0 < held <= 8 * F * 4 + 16 * 12, held
    _check(cut, one, "chunked against one chunk")
    _check(one, exp, "one chunk")


@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)               # several chunks, more than the pipeline has slots
    R, F = 64, 128
    reads, refs, _ = cases.fuzz_batch(5000, R, F, seed=12, plant_at=20)
    for form in ("sym", "aff"):
        eng = hipkernel.Engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs, 32)
        for threads in (1, 4):
            _check(_host(eng, reads, refs, 32, threads), dev, (form, threads, chunks))
        assert eng.describe(0, 5000)["direct_call"] == 0
        eng.set_host_packing(0)
        _check(_host(eng, reads, refs, 32, 2), dev, (form, "raw ASCII", chunks))
        _check(_host(eng, reads[:100], refs[:100], 32, 2), dev[:100], (form, "direct"))        # the direct call
        assert eng.describe(0, 100)["direct_call"] == 1
        eng.close()
    _check(dev[:256], subopt_ref.subopt(reads[:256], refs[:256], _scoring("aff"), 32, affine=True), "device path")


def test_two_calls_back_to_back_on_a_stream_of_their_own():
    R, F = 150, 500
    a_reads, a_refs, _ = cases.fuzz_batch(64, R, F, seed=21, plant_at=10)
    b_reads, b_refs, _ = cases.fuzz_batch(48, R, F, seed=22, plant_at=200)
    sc = _scoring("sym")
    eng = hipkernel.Engine(R, F, sc)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        ra, fa, rb, fb = (torch.from_numpy(x).cuda() for x in (a_reads, a_refs, b_reads, b_refs))
        out_a = eng.score_subopt_device(0, ra, fa, 75, stream=st)
        out_b = eng.score_subopt_device(0, rb, fb, 10, stream=st)       # reuses the scratch behind the first call's records
    st.synchronize()
    eng.close()
    _check(out_a.cpu().numpy().astype(np.int64), subopt_ref.subopt(a_reads, a_refs, sc, 75), "first call")
    _check(out_b.cpu().numpy().astype(np.int64), subopt_ref.subopt(b_reads, b_refs, sc, 10), "second call")


# ---- 7. consistency with placed scores ----
@pytest.mark.parametrize("form", list(FORMS))
def test_first_three_fields_are_the_placed_record(form):
    R, F = 150, 500
    reads, refs, _ = cases.fuzz_batch(64, R, F, seed=31, plant_at=77)
    rng = np.random.default_rng(1)
    reads = _trim_half(reads, rng)
    for match in (2, 14):                   # key and rows
        sc = _scoring(form, match)
        eng = hipkernel.Engine(R, F, sc)
        placed = eng.score_placed_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
        torch.cuda.synchronize()
        got = _run(eng, reads, refs, 40)
        d = eng.describe(0, 64)
        eng.close()
        assert d["ran_subopt"] == d["ran_placed"] == ("key" if match == 2 else "rows")
        assert np.array_equal(got[:, :3], placed.cpu().numpy().astype(np.int64)), (form, match)


# ---- 8. refusals ----
def test_refusals_and_the_silent_no_op():
    R, F = 150, 500
    reads, refs, _ = cases.fuzz_batch(8, R, F, seed=1)
    dr, df = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    sc = _scoring("sym")

    def refused(eng, text, opt=0, mask=5):
        with pytest.raises(hipkernel.HipKernelError, match=text):
            eng.score_subopt_device(opt, dr, df, mask)
        with pytest.raises(hipkernel.HipKernelError, match=text):
            eng.score_subopt_host(opt, reads, refs, mask)
        assert eng.describe(0, 8)["ran_subopt"] == "none"

    eng = hipkernel.Engine(R, F, sc)
    refused(eng, "need mask >= 0", mask=-1)
    refused(eng, "Smith-Waterman only", opt=1)
    # opt & 0xF > 1: nothing happens, nothing is written
    out = torch.full((8, 5), -7, dtype=torch.int32, device="cuda")
    eng.score_subopt_device(2, dr, df, 5, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    assert (_host_raw(eng, reads, refs, 2) == 0).all()
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    eng.set_score_width(32)
    refused(eng, "score_width = 32")
    eng.set_placed_wide(1)
    refused(eng, "score_width = 32")                     # placed_wide does not open the int32 sweep here
    eng.set_score_width(0)
    for band_placed in (0, 1):
        eng.set_band_placed(band_placed)
        eng.set_band_width(64)
        refused(eng, "suboptimal scores are not built for band_width > 0")
        eng.set_band_width(0)
    _check(_run(eng, reads, refs, 5), subopt_ref.subopt(reads, refs, sc, 5), "after the refusals")
    eng.close()
    big = hipkernel.Scoring.make(214, -1, -3, -3)
    for wide in (0, 1):
        eng = hipkernel.Engine(R, F, big)
        eng.set_placed_wide(wide)
        refused(eng, "int16 cells: shape x scoring can leave their range")
        eng.close()
    # the row strips: more than 1 024 rows
    R2, F2 = 1025, 1300
    reads, refs, _ = cases.fuzz_batch(4, R2, F2, seed=1)
    dr, df = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    eng = hipkernel.Engine(R2, F2, sc)
    refused(eng, "register sweep only")
    eng.close()


def _host_raw(eng, reads, refs, opt):
    got = eng.score_subopt_host(opt, reads, refs, 5)
    return np.stack([got[k] for k in hipkernel.subopt_dtype().names], axis=1)


# ---- the ring in the block's LDS: the placed plan counts the reference tables only, every wave of the suboptimal form carries
# 1 KiB more.  On a forced 16 x 10 the tables of four waves fill the 160 KiB at 3 500 columns, one wave's at 16 200 ----
LDS = 160 * 1024


def test_a_block_whose_rings_do_not_fit_runs_with_fewer_waves():
    R, F, n = 150, 3500, 20
    sc = _scoring("sym")
    reads, refs, _ = cases.fuzz_batch(n, R, F, seed=5, plant_at=1700)
    reads = _trim_half(reads, np.random.default_rng(5))
    eng = hipkernel.Engine(R, F, sc, group_lanes=16, rows_per_lane=10)
    d = eng.describe(0, n)
    # the placed plan: four waves whose tables fit, and whose tables and rings do not
    assert d["waves_per_block"] == 4 and d["lds_per_block"] <= LDS < d["lds_per_block"] + 4 * 1024, d
    assert n > d["pairs_per_wave"] * 2                   # more than one block of two waves
    got = _run(eng, reads, refs, 75)
    _check(_host(eng, reads, refs, 75), got, "host path")
    ran = eng.describe(0, n)["ran_subopt"]
    eng.close()
    assert ran == "key"
    _check(got, subopt_ref.subopt(reads, refs, sc, 75, chunk=n), "two waves a block")


def test_one_wave_without_room_for_its_ring_is_refused():
    R, F = 150, 16200
    reads, refs, _ = cases.fuzz_batch(8, R, F, seed=6)
    eng = hipkernel.Engine(R, F, _scoring("sym"), group_lanes=16, rows_per_lane=10)
    d = eng.describe(0, 8)
    assert d["waves_per_block"] == 1 and d["lds_per_block"] <= LDS < d["lds_per_block"] + 1024, d
    text = "no room for its column ring"
    with pytest.raises(hipkernel.HipKernelError, match=text):
        eng.score_subopt_device(0, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda(), 75)
    with pytest.raises(hipkernel.HipKernelError, match=text):
        eng.score_subopt_host(0, reads, refs, 75)
    assert eng.describe(0, 8)["ran_subopt"] == "none"
    eng.close()
