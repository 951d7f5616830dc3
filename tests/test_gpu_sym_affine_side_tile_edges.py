"""The 8 x 19 side tile (score_kernel<8, 19, kAlgSW, kGapAffineSym>, dp_kernels.hip.h) at the edges tests/test_gpu_sym_affine_side_tile.py
never takes it to.  Conventions as there: half-float cells off, every score compared EXACTLY with oracle.cpu_ref.score(..., affine=True),
the tile asserted through describe() (_ran_tile).  Every forced call is legal by the rule or refused on the host before a launch.  The
edges are computed here from a small restatement of the rule and of side_tile_wave_lds (cell_constants.h) AND asserted as literals;
tests/sym_affine_side_tile_rules_check.cpp pins the same literals to the headers.

  a. the tilted window's upper edge: B + x (rows + F - lead) + min(R, F) match + 1 <= 0x7BFF at its last match score, with the full
     score in the last cell (the largest tilt) and with an early maximum that rides the accumulators up to the top index -- a top
     index off by one trip (K = 19 rows), a lead counted wrongly, an accumulator that is moved on once too often leave the window
     here and nowhere else (tests/test_sym_affine_odd_tile_sweep.py SEES the operands of the same constructions on the CPU);
  b. the LDS budget's edge: F = 558 is two 4-wave blocks of 77,824 B to the byte, F = 559 is refused -- a budget, a granule or a
     stride off by one puts a third block's worth of LDS out of reach or the streams over their area;
  c. both sides of every step of the stream stride (F = 120 | 121, 248 | 249, 376 | 377, 504 | 505) and reference lengths that
     are no multiple of 4 (the set-up's rim loop next to its 8-byte stores): a stride that differs between host and kernel, a
     rim column written with the wrong width;
  d. waves whose references ALL end early (cols_used < F): the trip count and the remainder entry come from cols_used, the stream
     stride from F -- a stride taken from cols_used, a remainder taken from F, an empty wave that does not write zeros;
  e. device pointers that are not 16-byte aligned: the set-up stages whole 16-byte spans and re-derives the skew of reads and
     references separately -- a skew ignored, or one side's skew used for the other;
  f. long gaps in both directions on the tile, and one matching base per (row, column) over a whole trip and a trip plus one;
  g. the host-pointer chunk pipeline: large chunks on the tile on the slots' streams, a short last chunk on the latency plan."""
import numpy as np
import pytest

import test_sym_affine_tilted_sweep as frame
from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import GAPS, _args, _device, _gapped_pairs, _one_hot, _refused
from test_gpu_sym_affine_side_tile import ACCEPTED, FORMS, LARGE, _batch, _engine, _expected, _forced, _ran_tile, _unforced
from test_sym_affine_odd_tile_sweep import edge_quarters, side_tile_edge_match
from test_sym_affine_row_tables_sweep import needs_repair, rule_ok
from versalignlib_amd import build, hipkernel, host

pytestmark = pytest.mark.gpu

G, K, ROWS = 8, 19, 152
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
RULE_TEXT = "sym_affine_row_tables_ok"


# ---- the rule, restated (cell_constants.h, cell_rules.h) ----
def stream_stride(F):
    """bytes of one group's stream: 16 bits per column, 12 pad columns at either end, 8 (mod 64) dwords"""
    dw = (F + 2 * (G + 4) + 1) // 2
    return 4 * (dw + (G - dw) % 64)


def wave_lds(R, F):
    refs_area, raw_reads = (16 * F + 32 + 15) // 16 * 16, (16 * R + 32 + 15) // 16 * 16
    return refs_area + max(8 * stream_stride(F), raw_reads)


def lds_ok(lds_wave):
    """two 4-wave blocks, each rounded up to 2 KB, inside 152 KB"""
    return lds_wave > 0 and 2 * (-(-4 * lds_wave // 2048) * 2048) <= 152 * 1024


def tile_accepts(R, F, scoring):
    """sym_affine_side_tile_refusal(..., forced = true) == "" for an int16 symmetric affine Smith-Waterman call"""
    match, mismatch, gap_open, gap_ext = scoring
    o, x = -gap_open, -gap_ext
    if o < 0 or x < 0 or R > ROWS or not rule_ok(*scoring):
        return False
    hi = min(R, F) * max(match, mismatch, 0) + 1
    plain = 1024 + o + x + max(0, -mismatch, -match)
    if plain - 1024 > 1024 or plain + hi > frame.WINDOW[1]:
        return False
    if frame.tilt_bias(*scoring) + x * frame.tilt_top_index(R, F, G, K) + hi > frame.WINDOW[1]:
        return False
    return lds_ok(wave_lds(R, F))


def test_the_restated_rule_has_the_literals():
    assert [F for F in range(1, 2000) if lds_ok(wave_lds(150, F))][-1] == 558
    for R in (129, 150, 152):
        assert wave_lds(R, 558) == 19456 and wave_lds(R, 559) == 19472 and lds_ok(19456) and not lds_ok(19457)
    begins = [(F, stream_stride(F)) for F in range(1, 560) if F == 1 or stream_stride(F) != stream_stride(F - 1)]
    assert begins == [(1, 288), (121, 544), (249, 800), (377, 1056), (505, 1312)]
    assert tile_accepts(150, 500, ACCEPTED) and not tile_accepts(150, 500, (2, -3, -5, -1)) and not tile_accepts(150, 559, ACCEPTED)


def _score(eng, reads, refs, n=None):
    n = len(reads) if n is None else n
    return eng.score_device(host.SW, _device(np.ascontiguousarray(reads[:n])), _device(np.ascontiguousarray(refs[:n]))).cpu().numpy()


def _exact(got, exp, what):
    bad = np.nonzero(got != exp)[0]
    assert got.shape == exp.shape and not bad.size, what + (bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())


def _oracle(reads, refs, scoring):
    return cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)


def _raises_forced(R, F, scoring, reads, refs, text):
    with pytest.raises(hipkernel.HipKernelError, match=text):
        eng = _engine(R, F, scoring)
        try:
            _score(eng, reads, refs)
        finally:
            eng.close()


# ---- a. the tilted window's upper edge ----
# (R, F, mismatch, open, extend) -> the last match score the rule accepts on rows = 152, K = 19.  The tilt-dominated scoring
# puts 20 x 710 into the frame; its table bytes are 20 .. match + 40 + 4.
WINDOW_EDGES = {(152, 152, -1, -5, -1): 200, (152, 558, -1, -5, -1): 197, (150, 500, -1, -5, -1): 200,
                (152, 558, -20, -24, -20): 108, (133, 558, -20, -24, -20): 124}


def _edge_batch(R, F):
    """40 pairs in four quarters of 10 (edge_quarters): last, first, last with an N, first with an N"""
    quarters = {}
    for k in range(10):
        for name, read, ref, clean in edge_quarters(R, F, seed=1000 * R + F + k):
            assert clean != needs_repair(ref)
            quarters.setdefault(name, []).append((read, ref))
    order = ("last", "first", "last-N", "first-N")
    reads = np.ascontiguousarray(np.stack([p[0] for name in order for p in quarters[name]]))
    refs = np.ascontiguousarray(np.stack([p[1] for name in order for p in quarters[name]]))
    return reads, refs


@pytest.mark.parametrize("case", sorted(WINDOW_EDGES), ids=lambda c: "%dx%d_%d_%d_%d" % c)
def test_the_tilted_windows_upper_edge_on_the_tile(monkeypatch, case):
    R, F, mismatch, gap_open, gap_ext = case
    match = side_tile_edge_match(R, F, mismatch, gap_open, gap_ext)           # (asserts the byte rule and the plain window at match + 1)
    assert match == WINDOW_EDGES[case]
    at, past = (match, mismatch, gap_open, gap_ext), (match + 1, mismatch, gap_open, gap_ext)
    assert tile_accepts(R, F, at) and not tile_accepts(R, F, past) and rule_ok(*past)      # the refusal is the window's, not the bytes'
    reads, refs = _edge_batch(R, F)
    # the last match score inside: the tile, both forms (wave 0 is clean), the full score by construction (one base short of it: at least
    # the diagonal's R - 1 matches)
    exp = _oracle(reads, refs, at)
    assert (exp[:20] == R * match).all() and ((R - 1) * match <= exp[20:]).all() and (exp[20:] < R * match).all() and R * match <= 32767
    eng = _engine(R, F, at)
    got = _score(eng, reads, refs)
    d = eng.describe(host.SW, 40)
    eng.close()
    _exact(got, exp, case + (match,))
    _ran_tile(d, case)
    assert d["ran_score_sym_affine_form"] == "both", d
    # the first outside: refused with the rule's text where forced, another geometry and the same exactness where not
    _raises_forced(R, F, past, reads, refs, RULE_TEXT)
    debug_switches(monkeypatch, no_side_tile=None)
    exp = _oracle(reads, refs, past)
    assert (exp[:20] == R * (match + 1)).all()
    reps = LARGE // 40
    eng = _engine(R, F, past, forced=False)
    got = _score(eng, np.tile(reads, (reps, 1)), np.tile(refs, (reps, 1)))
    d = eng.describe(host.SW, LARGE)
    eng.close()
    assert reps * 40 == LARGE and d["ran_score_geometry"] not in ("8x19", "none") and d["ran_score_cells"] == "int16", d
    _exact(got, np.tile(exp, reps), case + (match + 1, d["ran_score_geometry"]))


# ---- b. the LDS budget's edge ----
@pytest.mark.parametrize("R", (150, 152))
def test_the_lds_budgets_edge(monkeypatch, R):
    assert lds_ok(wave_lds(R, 558)) and not lds_ok(wave_lds(R, 559)) and wave_lds(R, 558) == 19456
    batch = _batch(R, 558, 33)
    assert _expected(batch, ACCEPTED).max() > 0
    eng = _engine(R, 558, ACCEPTED)
    got = _score(eng, batch[0], batch[1])
    d = eng.describe(host.SW, 33)
    eng.close()
    _exact(got, _expected(batch, ACCEPTED), (R, 558, "forced"))
    _ran_tile(d, (R, 558))
    assert d["lds_per_block"] == 4 * 19456 and 2 * d["lds_per_block"] <= 152 * 1024, d
    _, d = _unforced(monkeypatch, R, 558, ACCEPTED)                  # 16,400 pairs, exact (asserted there)
    _ran_tile(d, (R, 558, "unforced"))
    assert d["lds_per_block"] == 4 * 19456 and (d["pairs_per_wave"], d["waves_per_block"]) == (16, 4), d
    # one column more: refused where forced, another geometry with exact scores where not
    batch = _batch(R, 559, 33)
    _raises_forced(R, 559, ACCEPTED, batch[0], batch[1], "too long for its LDS budget")
    _, d = _unforced(monkeypatch, R, 559, ACCEPTED)
    assert d["ran_score_geometry"] not in ("8x19", "none") and d["rows_per_lane"] != 19, d


# ---- c. the stream stride's steps and the rim ----
STRIDE_COLUMNS = (120, 121, 122, 123, 248, 249, 376, 377, 504, 505, 557, 558)


@pytest.mark.parametrize("R", (133, 152))
def test_both_sides_of_every_stride_step_and_the_rim(R):
    assert {stream_stride(F) for F in STRIDE_COLUMNS} == {288, 544, 800, 1056, 1312}
    assert {F % 4 for F in STRIDE_COLUMNS} == {0, 1, 2, 3}
    seen = set()
    for F in STRIDE_COLUMNS:
        assert stream_stride(F) != stream_stride(F + 1) or F not in (120, 248, 376, 504)
        batch = _batch(R, F, 33)
        assert _expected(batch, ACCEPTED).max() > 0
        seen.update(_forced(R, F, ACCEPTED, batch, (17, 33)))       # (a tail wave of one pair: pair B is missing everywhere in it)
    assert seen <= set(FORMS) and seen & {"row_tables", "both"} and seen & {"row_tables_repair", "both"}, seen


# ---- d. waves whose references all end early ----
def _planted(R, F, n, seed):
    """Clean ACGT pairs: the read is the reference's first bases less a deletion of 1 .. 3 (a shorter reference: planted whole
    in the read), so that every prefix of the reference and of the read scores something"""
    rng = np.random.default_rng(seed)
    refs = np.ascontiguousarray(ACGT[rng.integers(0, 4, size=(n, F))])
    reads = np.ascontiguousarray(ACGT[rng.integers(0, 4, size=(n, R))])
    for i in range(n):
        piece = refs[i, :R + 3]
        cut = int(rng.integers(8, piece.size - 4))
        piece = np.concatenate((piece[:cut], piece[cut + int(rng.integers(1, 4)):]))[:R]
        reads[i, :piece.size] = piece
    return reads, refs


@pytest.mark.parametrize("shape", ((150, 558), (152, 64)), ids=lambda s: "%dx%d" % s)
def test_waves_whose_references_all_end_early(shape):
    R, F = shape
    ends = [1, 2, 0] + list(range(3, 40)) + [F - 1, F]              # per wave; the all-empty wave sits between live ones
    assert len(ends) == 42 and {frame._remainder(R, c, G, K) for c in ends} == set(range(K)) and (ROWS - R) // K == 0
    assert stream_stride(F) == {558: 1312, 64: 288}[F]             # the stride is F's however short the sweep
    reads, refs = _planted(R, F, 16 * len(ends), seed=R + F)
    eng = _engine(R, F, ACCEPTED)
    for tail in (0, ord("N")):
        cut = refs.copy()
        for w, c in enumerate(ends):
            cut[16 * w:16 * w + 16, c:] = tail
        assert not any(needs_repair(r) for r in cut)
        exp = _oracle(reads, cut, ACCEPTED)
        live = np.repeat(np.array(ends) > 0, 16)
        assert (exp[live] > 0).all() and not exp[~live].any() and exp[-16:].min() > 100
        got = _score(eng, reads, cut)
        d = eng.describe(host.SW, len(reads))
        _exact(got, exp, (R, F, "references end early", tail))
        _ran_tile(d, (R, F, tail))
        assert d["ran_score_sym_affine_form"] == "row_tables", d
    # ... and waves whose READS all end early: live rows at the top of the padded read, the lead still the engine's
    lengths = (0, 1, 18, 19, 20, 132, 133)
    short = reads[:16 * len(lengths)].copy()
    for w, r in enumerate(lengths):
        short[16 * w:16 * w + 16, r:] = 0
    exp = _oracle(short, refs[:len(short)], ACCEPTED)
    assert not exp[:16].any() and (exp[16:] > 0).all() and exp[-16:].min() > 100
    got = _score(eng, short, refs[:len(short)])
    d = eng.describe(host.SW, len(short))
    eng.close()
    _exact(got, exp, (R, F, "reads end early"))
    _ran_tile(d, (R, F, "reads"))


# ---- e. device pointers that are not 16-byte aligned ----
def _offset_view(array, k, fill):
    """A contiguous device view of `array` that starts k bytes into a larger byte tensor full of `fill` (a base: whatever a
    wrong skew reads scores)"""
    import torch
    flat = torch.full((array.size + 64,), fill, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    view = flat[k:k + array.size].view(array.shape)
    view.copy_(torch.from_numpy(array))
    assert view.is_contiguous() and view.data_ptr() % 16 == k % 16
    return view


@pytest.mark.parametrize("shape", ((150, 121), (152, 558)), ids=lambda s: "%dx%d" % s)
def test_unaligned_device_pointers(shape):
    import torch
    R, F = shape
    batch = _batch(R, F, 33)
    reads, refs = batch[0].copy(), batch[1].copy()
    exp = _expected(batch, ACCEPTED)
    assert exp.max() > 0
    eng = _engine(R, F, ACCEPTED)
    aligned = _score(eng, reads, refs)
    _exact(aligned, exp, (R, F, "aligned"))
    for k_reads, k_refs in ((1, 3), (3, 1), (8, 13), (13, 8), (15, 15), (0, 15), (13, 0)):
        d_reads, d_refs = _offset_view(reads, k_reads, ord("G")), _offset_view(refs, k_refs, ord("G"))
        out = torch.full((34,), -7, dtype=torch.int16, device="cuda")              # the scores one element into a tensor
        assert out[1:].data_ptr() % 4 == 2
        eng.score_device(host.SW, d_reads, d_refs, scores=out[1:])
        got = out.cpu().numpy()
        d = eng.describe(host.SW, 33)
        _ran_tile(d, (R, F, k_reads, k_refs))
        assert got[0] == -7, got[0]
        _exact(got[1:], exp, (R, F, k_reads, k_refs))
        assert np.array_equal(got[1:], aligned)
    eng.close()


# ---- f. long gaps, and one matching base over a whole trip ----
GAP_SCORINGS = [sub + gaps for sub in ((2, -1), (5, -4)) for gaps in GAPS] + [(6, -2, -5, -1), (6, -2, -1, -1), (6, -2, -7, -3)]


@pytest.mark.parametrize("shape", ((150, 64), (152, 300), (129, 505)), ids=lambda s: "%dx%d" % s)
def test_long_gaps_on_the_tile(shape):
    R, F = shape
    reads, refs = _gapped_pairs(600, R, F, seed=1000 * R + F)
    ran = []
    for scoring in GAP_SCORINGS:
        if _refused(scoring):                                       # (open, extend) = (-2, -3): no affine model, no engine
            continue
        if not tile_accepts(R, F, scoring):
            _raises_forced(R, F, scoring, reads[:16], refs[:16], RULE_TEXT)
            continue
        exp = _oracle(reads, refs, scoring)
        if scoring == ACCEPTED and F >= R:
            assert (exp > 29 * scoring[0]).mean() > 0.5             # the gaps are used: no ungapped piece of a read has 30 bases
        assert exp.max() > 0
        eng = _engine(R, F, scoring)
        got = _score(eng, reads, refs)
        d = eng.describe(host.SW, 600)
        eng.close()
        _exact(got, exp, (R, F, scoring))
        _ran_tile(d, (R, F, scoring))
        ran.append(scoring)
    assert len(ran) >= 3 and ACCEPTED in ran, ran


@pytest.mark.parametrize("F", (19, 20))
def test_one_hot_over_a_whole_trip(F):
    R = 152
    reads, refs = _one_hot(R, F)
    eng = _engine(R, F, ACCEPTED)
    got = _score(eng, reads, refs)
    d = eng.describe(host.SW, R * F)
    eng.close()
    _ran_tile(d, (R, F))
    assert d["ran_score_sym_affine_form"] == "row_tables", d
    assert got.shape == (R * F,) and (got == ACCEPTED[0]).all(), np.nonzero(got != ACCEPTED[0])[0][:8]     # by construction
    _exact(got, _oracle(reads, refs, ACCEPTED), (R, F, "one hot"))


# ---- g. the host-pointer chunk pipeline ----
PLUGIN_SCORING = dict(score_match=2, score_mismatch=-1, score_gap_read=-3, score_gap_ref=-3, score_gap_open_read=-5, score_gap_extend_read=-1,
                      score_gap_open_ref=-5, score_gap_extend_ref=-1, half_float_cells=0, num_threads=4)
# (chunk pairs, call pairs) at 150 x 64, 214 bytes per pair.  A call of at most two chunks runs them as they are: one large chunk
# and a remainder of 400; two large chunks.  A longer call ramps up -- a quarter chunk, half a chunk, then whole ones -- so its
# chunk is 66,000 pairs: 16,500, 33,000, 66,000, 66,000 and a remainder of 400, every chunk but the last beyond the latency plan.
HOST_CALLS = {"remainder": (39600, 40000), "two-large": (20000, 40000), "ramp": (66000, 181900)}


def _host_data(n):
    batch = _batch(150, 64, 400, seed=3)
    reps = -(-n // 400)
    return np.tile(batch[0], (reps, 1))[:n].copy(), np.tile(batch[1], (reps, 1))[:n].copy(), np.tile(_expected(batch, ACCEPTED), reps)[:n]


@pytest.mark.parametrize("call", sorted(HOST_CALLS))
def test_the_host_path_runs_its_large_chunks_on_the_tile(monkeypatch, call):
    chunk, n = HOST_CALLS[call]
    few = LARGE - 16                                                # the most pairs any latency plan takes
    if call == "ramp":
        assert n > 2 * chunk and chunk // 4 > few and n - chunk // 4 - chunk // 2 - 2 * chunk == 400
    else:
        assert n <= 2 * chunk and chunk > few and n - chunk in (400, chunk)
    reads, refs, exp = _host_data(n)
    assert exp.max() > 0
    described = {}
    for side in (True, False):
        debug_switches(monkeypatch, chunk_bytes=214 * chunk, no_side_tile=None if side else 1)
        eng = _engine(150, 64, ACCEPTED, forced=False)
        got = eng.score_host(host.SW, reads, refs, threads=4)
        described[side] = eng.describe(host.SW, n)
        eng.close()
        _exact(got, exp, (call, "flat", side))
        if call == "ramp":
            continue
        with host.Plugin(build.HIP_PLUGIN, 150, 64, **PLUGIN_SCORING) as plug:
            got = plug.score_alignments(host.SW, reads, refs)
            ran = plug.last_ran()
        _exact(got, exp, (call, "plugin", side))
        assert ran and ran["ran_score_cells"] == "int16", ran
    d, d_off = described[True], described[False]
    assert d["direct_call"] == 0 and d["ran_score_cells"] == "int16" and d_off["ran_score_geometry"] not in ("8x19", "none"), (d, d_off)
    if call == "two-large":                                         # the last chunk is a large one: what describe() reports is the tile
        _ran_tile(d, (call,))
        assert d["ran_score_sym_affine_form"] in FORMS, d
    else:                                                           # the last chunk of 400 took the latency plan
        assert d["ran_score_geometry"] not in ("8x19", "none"), d
