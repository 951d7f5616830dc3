"""Extension scores on the GPU (valign_hip_score_extend_device / _host): the anchored score, its end cell and the read-end score
from one sweep with gap-priced borders and no floor, against tests/extend_ref.py (numpy, int64 cells, the whole matrix,
independent of the library).  Integers, compared exactly, all five fields."""
import numpy as np
import pytest
import torch

import extend_ref
import instance_matrix as im
from conftest import debug_switches
from versalignlib_amd import hipkernel

pytestmark = pytest.mark.gpu

FULL = [(8, 8), (16, 10), (32, 10), (64, 8), (64, 16), (64, 32)]
# linear symmetric, linear gap_read != gap_ref, affine symmetric, affine with four scores
FORMS = {"sym": (-3, -3), "lin": (-2, -4), "affsym": (-3, -3, -5, -1, -5, -1), "aff": (-3, -3, -6, -2, -4, -1)}
BASES = np.frombuffer(b"ACGT", np.uint8)


def _scoring(form, match=2, mismatch=-1):
    return hipkernel.Scoring.make(match, mismatch, *FORMS[form])


def _affine(form):
    return len(FORMS[form]) > 2


def _run(eng, reads, refs, opt=0):
    out = eng.score_extend_device(opt, torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


def _host(eng, reads, refs, threads=1):
    got = eng.score_extend_host(0, reads, refs, threads=threads)
    assert got.dtype == hipkernel.extend_dtype() and got.shape == (len(reads),)
    return np.stack([got[k] for k in hipkernel.extend_dtype().names], axis=1).astype(np.int64)


def _check(got, exp, what):
    bad = np.nonzero((got != exp).any(axis=1))[0]
    assert bad.size == 0, (what, "pairs", bad[:8].tolist(), "got", got[bad[:4]].tolist(), "expected", exp[bad[:4]].tolist())


def _batch(n, R, F, seed, trim=True):
    """Extensions from the anchor of a random length, with a mismatch or a gap on the way in some; half of the reads and half of
    the references trimmed to random lengths (N or NUL), so that the two halves of a packed register differ in Rp and Fp."""
    rng = np.random.default_rng(seed)
    reads, refs = BASES[rng.integers(0, 4, (n, R))], BASES[rng.integers(0, 4, (n, F))]
    for p in range(n):
        L = int(rng.integers(1, min(R, F) + 1))
        kind = p % 4
        if kind == 0:
            refs[p, :L] = reads[p, :L]
        elif kind == 1 and F > 3:                       # the reference carries extra bases in the middle
            cut, extra = L // 2, int(rng.integers(1, 3))
            refs[p, :cut] = reads[p, :cut]
            tail = min(L - cut, F - cut - extra)
            if tail > 0:
                refs[p, cut + extra:cut + extra + tail] = reads[p, cut:cut + tail]
        elif kind == 2 and R > 3:                       # the read carries extra bases in the middle
            cut, extra = L // 2, int(rng.integers(1, 3))
            refs[p, :cut] = reads[p, :cut]
            tail = min(L - cut - extra, F - cut)
            if tail > 0:
                refs[p, cut:cut + tail] = reads[p, cut + extra:cut + extra + tail]
        if trim and p % 2 == 0:
            reads[p, int(rng.integers(1, R + 1)):] = rng.choice([0, ord("N")])
        if trim and (p // 2) % 2 == 0:
            refs[p, int(rng.integers(1, F + 1)):] = rng.choice([0, ord("N")])
    return reads, refs


# ---- 1. every compiled instance: six full geometries x four gap forms, at the instance matrix's shapes ----
@pytest.mark.parametrize("shape", range(4))
@pytest.mark.parametrize("G,K", FULL)
def test_every_instance(G, K, shape):
    n = im.batch(G)
    R, F = im.shapes(G, K)[shape]
    reads, refs = _batch(n, R, F, seed=G * K + shape)
    for form in FORMS:
        sc = _scoring(form)
        exp = extend_ref.extend(reads, refs, sc, affine=_affine(form), chunk=16)
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        got = _run(eng, reads, refs)
        d = eng.describe(0, n)
        eng.close()
        _check(got, exp, (G, K, R, F, form))
        assert d["ran_extend"] == "rows", (G, K, R, F, form, d["ran_extend"])
        assert d["ran_extend_geometry"] == "%dx%d" % (G, K), (G, K, R, F, form, d["ran_extend_geometry"])
    assert (exp[:, 0] > 0).any() and (exp[:, 3] < 0).any()


# ---- 2. border cases ----
GEOS = [(8, 8), (16, 10)]


def _border_cases(R, F):
    rng = np.random.default_rng(R * F)
    reads, refs, names = [], [], []

    def add(name, rd, rf):
        assert len(rd) == R and len(rf) == F
        reads.append(np.asarray(rd, np.uint8))
        refs.append(np.asarray(rf, np.uint8))
        names.append(name)

    core = BASES[rng.integers(0, 4, R)]
    junk = np.full(F, ord("T"), np.uint8)
    for extra in (1, 2, 3):
        # the reference begins with extra bases: the path starts in the border row
        rf = junk.copy()
        rf[:extra] = BASES[(np.searchsorted(BASES, core[:extra]) + 1) % 4]
        rf[extra:extra + min(R, F - extra)] = core[:min(R, F - extra)]
        add("ref+%d" % extra, core, rf)
        # the read begins with extra bases: the path starts in the border column
        rd = core.copy()
        rf = junk.copy()
        rf[:min(R - extra, F)] = core[extra:extra + min(R - extra, F)]
        rd[:extra] = BASES[(np.searchsorted(BASES, rf[:extra]) + 2) % 4]
        add("read+%d" % extra, rd, rf)
    # first bases all mismatching: an empty record with a negative gscore
    add("all mismatch", np.full(R, ord("A"), np.uint8), np.full(F, ord("C"), np.uint8))
    # the read longer than the trimmed reference: the padding columns are no candidates
    rf = np.zeros(F, np.uint8)
    rf[:R // 2] = core[:R // 2]
    add("read beyond Fp", core, rf)
    rf = np.full(F, ord("N"), np.uint8)
    rf[:R // 3] = core[:R // 3]
    add("read beyond Fp (N)", core, rf)
    # Rp in {0, 1, R} x Fp in {0, 1, F}
    for Rp in (0, 1, R):
        for Fp in (0, 1, F):
            rd, rf = np.zeros(R, np.uint8), np.full(F, ord("N"), np.uint8)
            rd[:Rp] = core[:Rp]
            k = min(Rp, Fp)
            rf[:Fp] = BASES[rng.integers(0, 4, Fp)]
            rf[:k] = core[:k]
            add("Rp %d Fp %d" % (Rp, Fp), rd, rf)
    # an interior N and a byte >= 0x80
    rd, rf = core.copy(), junk.copy()
    rf[:min(R, F)] = core[:min(R, F)]
    rd[R // 2] = ord("N")
    rf[R // 4] = 0x9C
    add("interior junk", rd, rf)
    rd2 = core.copy()
    rd2[R // 3] = 0xFF
    rf2 = rf.copy()
    rf2[R // 4] = ord("n")
    add("interior junk 2", rd2, rf2)
    return np.stack(reads), np.stack(refs), names


@pytest.mark.parametrize("G,K", GEOS)
@pytest.mark.parametrize("R,F", [(12, 20), (33, 70)])
def test_border_cases(R, F, G, K):
    reads, refs, names = _border_cases(R, F)
    assert len(reads) % 2 == 0
    for form in FORMS:
        sc = _scoring(form)
        exp = extend_ref.extend(reads, refs, sc, affine=_affine(form))
        by_name = dict(zip(names, exp.tolist()))
        assert by_name["all mismatch"][:3] == [0, 0, 0] and by_name["all mismatch"][3] < 0
        assert by_name["Rp 0 Fp %d" % F] == [0, 0, 0, 0, 0] and by_name["read beyond Fp"][4] <= R // 2
        assert by_name["ref+2"][0] > 0 and by_name["read+2"][0] > 0
        eng = hipkernel.Engine(R, F, sc, group_lanes=G, rows_per_lane=K)
        _check(_run(eng, reads, refs), exp, (R, F, G, K, form))
        # n odd and a partial wave: one pair, three pairs, and all but the last
        for n in (1, 3, len(reads) - 1):
            _check(_run(eng, reads[:n], refs[:n]), exp[:n], (R, F, G, K, form, "n", n))
        eng.close()


# ---- 3. one size-up: 150 x 500, the host entry with 1 and 4 threads against the device entry ----
@pytest.mark.parametrize("form", ["sym", "aff"])
def test_size_up_host_and_device(form):
    R, F, n = 150, 500, 512
    reads, refs = _batch(n, R, F, seed=11)
    sc = _scoring(form)
    eng = hipkernel.Engine(R, F, sc)
    dev = _run(eng, reads, refs)
    assert eng.describe(0, n)["ran_extend"] == "rows"
    _check(dev[:96], extend_ref.extend(reads[:96], refs[:96], sc, affine=_affine(form), chunk=32), (form, "device"))
    for threads in (1, 4):
        _check(_host(eng, reads, refs, threads), dev, (form, "host", threads))
    eng.close()


# ... and the host entry's chunk pipeline: several chunks (more than it has slots), 4-bit classes and raw ASCII, the direct call
@pytest.mark.parametrize("chunks", [False, True])
def test_host_path_equals_device_path(monkeypatch, chunks):
    if chunks:
        debug_switches(monkeypatch, chunk_bytes=200000)
    R, F, n = 64, 128, 5000
    reads, refs = _batch(n, R, F, seed=12)
    for form in ("lin", "affsym"):
        eng = hipkernel.Engine(R, F, _scoring(form))
        dev = _run(eng, reads, refs)
        for threads in (1, 4):
            _check(_host(eng, reads, refs, threads), dev, (form, threads, chunks))
        assert eng.describe(0, n)["direct_call"] == 0
        eng.set_host_packing(0)
        _check(_host(eng, reads, refs, 2), dev, (form, "raw ASCII", chunks))
        _check(_host(eng, reads[:100], refs[:100], 2), dev[:100], (form, "direct"))
        assert eng.describe(0, 100)["direct_call"] == 1
        eng.close()
    _check(dev[:256], extend_ref.extend(reads[:256], refs[:256], _scoring("affsym"), affine=True), "device path")


# ---- 4. refusals ----
def test_refusals():
    R, F = 33, 70
    reads, refs = _batch(4, R, F, seed=3)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()

    def refused(eng, word, opt=0, rd=d_reads, rf=d_refs, host=(reads, refs)):
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_device(opt, rd, rf)
        assert eng.describe(0, 4)["ran_extend"] == "none"
        with pytest.raises(hipkernel.HipKernelError, match=word):
            eng.score_extend_host(opt, host[0], host[1])
        assert eng.describe(0, 4)["ran_extend"] == "none"

    sc = _scoring("sym")
    eng = hipkernel.Engine(R, F, sc)
    assert _run(eng, reads, refs).shape == (4, 5) and eng.describe(0, 4)["ran_extend"] == "rows"
    refused(eng, "opt & 0xF == 0 only", opt=1)
    # opt & 0xF > 1 does nothing
    out = torch.full((4, 5), -7, dtype=torch.int32, device="cuda")
    eng.score_extend_device(2, d_reads, d_refs, out=out)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7).all()
    eng.set_traceback_policy(1)
    refused(eng, "traceback_policy = 1")
    eng.set_traceback_policy(0)
    for band_placed in (0, 1):
        eng.set_band_placed(band_placed)
        eng.set_band_width(16)
        refused(eng, "not built for band_width > 0")
        eng.set_band_width(0)
    eng.set_band_placed(0)
    for wide in (0, 1):
        eng.set_placed_wide(wide)
        eng.set_score_width(32)
        refused(eng, "score_width = 32")
        eng.set_score_width(0)
    eng.set_placed_wide(0)
    _check(_run(eng, reads, refs), extend_ref.extend(reads, refs, sc), "after the refusals")
    eng.close()
    # cells that could leave int16: the top (33 x 970 > 32000) and the bottom (103 gap steps at -320)
    for scoring in (hipkernel.Scoring.make(970, -1, -3, -3), hipkernel.Scoring.make(2, -1, -320, -320)):
        for wide in (0, 1):
            eng = hipkernel.Engine(R, F, scoring)
            eng.set_placed_wide(wide)
            refused(eng, "signed int16 cells")
            eng.close()
    # the row strips: an unforced 1 500 x 1 500 call
    big = np.full((2, 1500), ord("A"), np.uint8)
    eng = hipkernel.Engine(1500, 1500, sc)
    refused(eng, "register sweep only", rd=torch.from_numpy(big).cuda(), rf=torch.from_numpy(big).cuda(), host=(big, big))
    eng.close()


# ---- 5. invariants on the device's own output ----
@pytest.mark.parametrize("form", ["lin", "affsym"])
def test_invariants_against_placed_scores(form):
    R, F, n = 100, 260, 301
    reads, refs = _batch(n, R, F, seed=29)
    sc = _scoring(form)
    eng = hipkernel.Engine(R, F, sc)
    d_reads, d_refs = torch.from_numpy(reads).cuda(), torch.from_numpy(refs).cuda()
    ext = eng.score_extend_device(0, d_reads, d_refs)
    placed = eng.score_placed_device(0, d_reads, d_refs)
    torch.cuda.synchronize()
    ext, placed = ext.cpu().numpy().astype(np.int64), placed.cpu().numpy().astype(np.int64)
    eng.close()
    assert (ext[:, 0] <= placed[:, 0]).all()
    Fp, Rp = extend_ref.trimmed_lengths(refs), extend_ref.trimmed_lengths(reads)
    assert (ext[Fp > 0, 3] <= ext[Fp > 0, 0]).all()
    assert (ext[:, 1] <= Rp).all() and (ext[:, 2] <= Fp).all() and (ext[:, 4] <= Fp).all() and (ext[:, 4] >= 0).all()
    assert ((ext[:, 0] == 0) == (ext[:, 1] == 0)).all() and ((ext[:, 0] == 0) == (ext[:, 2] == 0)).all()
