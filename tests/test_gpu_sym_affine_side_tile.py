"""The 8 x 19 side tile of the tilted int16 Smith-Waterman sweep with symmetric affine gaps (score_kernel<8, 19, kAlgSW,
kGapAffineSym>, dp_kernels.hip.h; the rule: cell_rules.h, sym_affine_side_tile_refusal; tests/test_sym_affine_odd_tile_sweep.py
restates its step on the CPU).  Half-float cells are off everywhere; every score is compared EXACTLY with oracle.cpu_ref.score and
describe() says which geometry ran (ran_score_geometry) and where the scores came from (ran_score_sym_affine_scores).

  a. the tile forced, reads of 132, 133, 150, 151 and 152 bases (a padding lane and a row, that lane exactly, one padding row,
     none; the unpaired row 18 is real in all of them) against references of 1, 2, 7, 8, 9, 18, 19, 20, 37, 38 and 39 bases
     (sweeps shorter than the skew, step counts = 0, 1 and K - 1 mod K: every remainder entry), batches of 1, 15, 16, 17 and 33
     pairs (a lone pair, a missing pair B, a full wave, a tail wave, a tail into the third wave), with the scoring of
     tests/test_gpu_sym_affine_row_tables.py and one at each byte edge of the rule;
  b. reads of 129 bases and of 1 base, forced: only the last lane, or only its last row, is live;
  c. one-hot batches at 152 x 5 and 152 x 6: one matching base per (row, column), everything else a mismatch;
  d. bases that are no ACGT: an N run before a reference's last ACGT base in every pair -- every wave runs the repairing form, and
     describe() says so (ran_score_sym_affine_form: the kernel reports the form each wave took) --, an N run after it and
     NUL-padded short reads and references: the plain form and no other; a batch that mixes them: both;
  e. length-sorted batches (ragged mode 2) of mixed lengths at 150 x 64: the scores of mode 0;
  f. selection without a forced geometry."""
import numpy as np
import pytest

from conftest import debug_switches
from oracle import cpu_ref
from test_gpu_sym_affine_max3 import _args, _device, _one_hot
from test_sym_affine_row_tables_sweep import needs_repair
from versalignlib_amd import hipkernel, host

pytestmark = pytest.mark.gpu

TILE = (8, 19)
ACCEPTED = (2, -1, -5, -1)          # the benchmark's scoring: x = 1, o - x = 4, match' 4, mismatch' 1, zero' 2
REFUSED = (2, -3, -5, -1)           # mismatch' = -1: no byte
LOW_EDGE = (2, -2, -5, -1)          # mismatch' = 0, the smallest byte
HIGH_EDGE = (249, -1, -5, -1)       # match' + (o - x) = 255, the largest byte (short references: inside the tilted window)
COLUMNS = (1, 2, 7, 8, 9, 18, 19, 20, 37, 38, 39)
PAIRS = (1, 15, 16, 17, 33)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

FORMS = ("row_tables", "row_tables_repair", "both")
_cache = {}


def _batch(R, F, n, seed=0, dirt=True):
    """n pairs: a mutated piece of the reference planted in the read; with `dirt`, every third pair an N inside its reference, every
    fourth an N run in its read, every fifth NUL tails.  Cached (read-only) with its oracle scores per scoring."""
    key = (R, F, n, seed, dirt)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(7919 * R + 104729 * F + seed)
    refs = np.ascontiguousarray(ACGT[rng.integers(0, 4, size=(n, F))])
    reads = np.ascontiguousarray(ACGT[rng.integers(0, 4, size=(n, R))])
    for i in range(n):
        piece = refs[i, int(rng.integers(0, max(1, F // 3))):][:R].copy()
        if piece.size > 6:
            cut = int(rng.integers(1, piece.size - 4))
            piece = np.concatenate((piece[:cut], piece[cut + int(rng.integers(1, 4)):]))
            piece[int(rng.integers(0, piece.size))] = ACGT[int(rng.integers(0, 4))]
        at = int(rng.integers(0, R - piece.size + 1))
        reads[i, at:at + piece.size] = piece
        if not dirt:
            continue
        if i % 3 == 1:
            refs[i, int(rng.integers(0, F))] = ord("N")
        if i % 4 == 2 and R > 1:
            a = int(rng.integers(0, R - 1))
            reads[i, a:a + int(rng.integers(1, 13))] = ord("N")
        if i % 5 == 3:
            refs[i, int(rng.integers(1, F + 1)):] = 0
            reads[i, int(rng.integers(1, R + 1)):] = 0
    reads.setflags(write=False)
    refs.setflags(write=False)
    _cache[key] = (reads, refs, {})
    return _cache[key]


def _expected(batch, scoring, alg=host.SW):
    reads, refs, oracle = batch
    if (scoring, alg) not in oracle:
        exp = cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*_args(scoring)), threads=4, affine=True)
        exp.setflags(write=False)
        oracle[(scoring, alg)] = exp
    return oracle[(scoring, alg)]


def _engine(R, F, scoring, forced=True):
    eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(scoring)), group_lanes=TILE[0] if forced else 0, rows_per_lane=TILE[1] if forced else 0)
    eng.set_half_float_cells(0)
    return eng


def _ran_tile(d, what):
    assert d["ran_score_cells"] == "int16" and d["ran_score_geometry"] == "8x19", what + (d["ran_score_geometry"],)
    assert d["ran_score_sym_affine"] == "max3" and d["ran_score_sym_affine_frame"] == "tilted", what
    assert d["ran_score_sym_affine_scores"] == "row_tables", what


def _forced(R, F, scoring, batch, counts, form=None):
    """form: what ran_score_sym_affine_form must say after every call (None: one of the three it can); -> what it said, per call"""
    reads, refs, _ = batch
    exp = _expected(batch, scoring)
    eng = _engine(R, F, scoring)
    seen = []
    for n in counts:
        got = eng.score_device(host.SW, _device(reads[:n].copy()), _device(refs[:n].copy())).cpu().numpy()
        what = (R, F, scoring, n)
        bad = np.nonzero(got != exp[:n])[0]
        assert not bad.size, what + (bad[:8].tolist(), got[bad[:8]].tolist(), exp[bad[:8]].tolist())
        d = eng.describe(host.SW, n)
        _ran_tile(d, what)
        assert d["ran_score_sym_affine_form"] == form if form else d["ran_score_sym_affine_form"] in FORMS, what + (d["ran_score_sym_affine_form"],)
        seen.append(d["ran_score_sym_affine_form"])
    eng.close()
    return seen


# ---- a. rows x columns x pairs ----
@pytest.mark.parametrize("scoring", (ACCEPTED, LOW_EDGE, HIGH_EDGE), ids=("bench", "low-edge", "high-edge"))
@pytest.mark.parametrize("R", (132, 133, 150, 151, 152))
def test_rows_columns_and_pairs(R, scoring):
    for F in COLUMNS:
        batch = _batch(R, F, max(PAIRS))
        assert _expected(batch, scoring).max() > 0
        _forced(R, F, scoring, batch, PAIRS)


# ---- b. only the last lane, or only its last row, is live ----
@pytest.mark.parametrize("R", (129, 1))
def test_short_reads_forced(R):
    for F in (1, 8, 20, 39):
        _forced(R, F, ACCEPTED, _batch(R, F, 17), (17, 1))


# ---- c. one matching base at (row i, column j): the score can come from that cell alone ----
@pytest.mark.parametrize("F", (5, 6))
def test_one_hot(F):
    R = 152
    reads, refs = _one_hot(R, F)
    eng = _engine(R, F, ACCEPTED)
    got = eng.score_device(host.SW, _device(reads), _device(refs)).cpu().numpy()
    d = eng.describe(host.SW, R * F)
    _ran_tile(d, (R, F))
    assert d["ran_score_sym_affine_form"] == "row_tables", d
    eng.close()
    assert got.shape == (R * F,) and (got == ACCEPTED[0]).all(), np.nonzero(got != ACCEPTED[0])[0][:8]     # by construction
    exp = cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(ACCEPTED)), threads=4, affine=True)
    assert np.array_equal(got, exp)


# ---- d. bases that are no ACGT ----
def _dirty(kind, R=150, F=64, n=48):
    reads, refs, _ = _batch(R, F, n, seed=11, dirt=False)
    reads, refs = reads.copy(), refs.copy()
    rng = np.random.default_rng(5 + len(kind))
    for i in range(n):
        if kind == "before":                    # an N run that ends before the reference's last ACGT base: every pair, so every wave repairs
            a = int(rng.integers(0, F - 6))
            refs[i, a:a + int(rng.integers(1, 5))] = ord("N")
            assert needs_repair(refs[i])
        elif kind == "after":                   # ... after it: the plain row-table step
            refs[i, int(rng.integers(F // 2, F)):] = ord("N")
            assert not needs_repair(refs[i])
        else:                                   # NUL-padded short reads and references
            refs[i, int(rng.integers(1, F + 1)):] = 0
            reads[i, int(rng.integers(1, R + 1)):] = 0
            assert not needs_repair(refs[i])
    return reads, refs, {}


@pytest.mark.parametrize("kind", ("before", "after", "nul"))
def test_bases_that_score_nothing(kind):
    batch = _dirty(kind)
    assert _expected(batch, ACCEPTED).max() > 0
    _forced(150, 64, ACCEPTED, batch, (48, 17), form="row_tables_repair" if kind == "before" else "row_tables")


def test_a_mixed_batch_runs_both_forms_and_each_call_reports_its_own():
    """Waves 0 and 2 of 48 pairs are clean, wave 1 has an N inside a reference: both; the first 16 pairs alone: the plain form --
    the words of a call do not survive into the next."""
    reads, refs, _ = _batch(150, 64, 48, seed=11, dirt=False)
    refs = refs.copy()
    refs[20, 10:13] = ord("N")
    assert needs_repair(refs[20]) and not any(needs_repair(r) for r in np.delete(refs, 20, axis=0))
    batch = (reads, refs, {})
    _forced(150, 64, ACCEPTED, batch, (48,), form="both")
    eng = _engine(150, 64, ACCEPTED)
    seen = []
    for n in (48, 16, 32):
        eng.score_device(host.SW, _device(reads[:n].copy()), _device(refs[:n].copy()))
        seen.append(eng.describe(host.SW, n)["ran_score_sym_affine_form"])
    eng.close()
    assert seen == ["both", "row_tables", "both"], seen


# ---- e. length-sorted batches: the read class of 129 .. 150 bases runs on the tile ----
def test_ragged_mode_2_is_mode_0(monkeypatch):
    debug_switches(monkeypatch, ragged_min=64)
    R, F, n = 150, 64, 640
    reads, refs, _ = _batch(R, F, n, seed=23, dirt=False)
    reads, refs = reads.copy(), refs.copy()
    rng = np.random.default_rng(23)
    for i in range(n):                          # trimmed read lengths of 20 .. 150, reference lengths of 10 .. 64
        if i % 3:
            reads[i, int(rng.integers(20, R + 1)):] = 0
        if i % 2:
            refs[i, int(rng.integers(10, F + 1)):] = 0
    exp = cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(ACCEPTED)), threads=4, affine=True)
    eng = _engine(R, F, ACCEPTED, forced=False)
    plain = eng.score_device(host.SW, _device(reads), _device(refs)).cpu().numpy()
    assert eng.describe(host.SW, n)["ragged_launches"] == 0
    eng.set_ragged_batching(2)
    sorted_ = eng.score_device(host.SW, _device(reads), _device(refs)).cpu().numpy()
    d = eng.describe(host.SW, n)
    eng.close()
    assert d["ragged_launches"] > 1 and d["ran_score_geometry"] == "8x19", d      # (the last launch: the longest read class)
    assert np.array_equal(sorted_, plain) and np.array_equal(plain, exp)


# ---- f. selection ----
LARGE = 16400           # more pairs than any latency plan takes (16 pairs per wave x 1024)


def _unforced(monkeypatch, R, F, scoring, alg=host.SW, switch=False, affine=True):
    debug_switches(monkeypatch, no_side_tile=1 if switch else None)
    batch = _batch(R, F, 400, seed=3)
    reads, refs, _ = batch
    reps = -(-LARGE // 400)
    big_reads, big_refs = np.tile(reads, (reps, 1))[:LARGE].copy(), np.tile(refs, (reps, 1))[:LARGE].copy()
    if affine:
        eng = _engine(R, F, scoring, forced=False)
        exp = _expected(batch, scoring, alg)
    else:
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*scoring))
        eng.set_half_float_cells(0)
        exp = cpu_ref.score(alg, reads, refs, cpu_ref.Scoring.make(*scoring), threads=4)
    got = eng.score_device(alg, _device(big_reads), _device(big_refs)).cpu().numpy()
    d = eng.describe(alg, LARGE)
    eng.close()
    assert np.array_equal(got, np.tile(exp, reps)[:LARGE]), (R, F, scoring, alg, np.nonzero(got != np.tile(exp, reps)[:LARGE])[0][:8])
    return got, d


@pytest.mark.parametrize("shape", ((150, 500), (151, 300), (129, 100)), ids=lambda s: "%dx%d" % s)
def test_eligible_shapes_take_the_tile(monkeypatch, shape):
    _, d = _unforced(monkeypatch, *shape, ACCEPTED)
    _ran_tile(d, shape)
    assert d["ran_score_sym_affine_form"] == "row_tables_repair", d    # (every third pair has an N inside its reference: no wave is clean)
    assert (d["group_lanes"], d["rows_per_lane"], d["pairs_per_wave"], d["waves_per_block"]) == (8, 19, 16, 4), d
    assert 2 * d["lds_per_block"] <= 152 * 1024, d


@pytest.mark.parametrize("shape", ((128, 500), (153, 500)), ids=lambda s: "%dx%d" % s)
def test_other_read_lengths_do_not(monkeypatch, shape):
    _, d = _unforced(monkeypatch, *shape, ACCEPTED)
    assert d["ran_score_geometry"] != "8x19" and d["rows_per_lane"] != 19, d


def test_a_score_that_is_no_byte_falls_back_to_the_lds_profile(monkeypatch):
    _, d = _unforced(monkeypatch, 150, 500, REFUSED)
    assert d["ran_score_geometry"] == "16x10" and d["ran_score_sym_affine_scores"] == "lds_profile", d


def test_linear_gaps_and_the_nw_variant_are_unaffected(monkeypatch):
    _, d = _unforced(monkeypatch, 150, 500, (2, -1, -3, -3), affine=False)
    assert d["ran_score_geometry"] not in ("8x19", "none") and d["rows_per_lane"] != 19 and "ran_score_sym_affine" not in d, d
    _, d = _unforced(monkeypatch, 150, 500, ACCEPTED, alg=host.NW)
    assert d["ran_score_geometry"] not in ("8x19", "none") and d["rows_per_lane"] != 19 and "ran_score_sym_affine" not in d, d


def test_the_debug_word_gives_the_old_plan_and_the_same_scores(monkeypatch):
    old, d_old = _unforced(monkeypatch, 150, 500, ACCEPTED, switch=True)
    assert d_old["ran_score_geometry"] == "16x10" and d_old["ran_score_sym_affine_scores"] == "row_tables", d_old
    new, d_new = _unforced(monkeypatch, 150, 500, ACCEPTED)
    _ran_tile(d_new, ("after the switch",))
    assert np.array_equal(old, new)


def test_small_calls_keep_the_latency_plan(monkeypatch):
    debug_switches(monkeypatch, no_side_tile=None)
    batch = _batch(150, 64, 48, seed=11, dirt=False)
    eng = _engine(150, 64, ACCEPTED, forced=False)
    got = eng.score_device(host.SW, _device(batch[0].copy()), _device(batch[1].copy())).cpu().numpy()
    d = eng.describe(host.SW, 48)
    eng.close()
    assert np.array_equal(got, _expected(batch, ACCEPTED)) and d["ran_score_geometry"] != "8x19", d


@pytest.mark.parametrize("case", ("byte", "half-floats", "nw", "read"))
def test_forcing_an_ineligible_call_raises_the_rules_text(case):
    R, F = (153, 64) if case == "read" else (150, 64)
    reads, refs, _ = _batch(R, F, 16)
    text = {"byte": "sym_affine_row_tables_ok", "half-floats": "int16 cells with symmetric affine gaps only", "nw": "Smith-Waterman scores only",
            "read": "does not fit"}[case]
    with pytest.raises(hipkernel.HipKernelError, match=text):
        eng = hipkernel.Engine(R, F, hipkernel.Scoring.make(*_args(REFUSED if case == "byte" else ACCEPTED)), group_lanes=8, rows_per_lane=19)
        try:
            if case != "half-floats":
                eng.set_half_float_cells(0)
            eng.score_device(host.NW if case == "nw" else host.SW, _device(reads.copy()), _device(refs.copy()))
        finally:
            eng.close()
