"""The 8 x 19 side tile (score_kernel<8, 19, kAlgSW, kGapAffineSym>, dp_kernels.hip.h) under its INTERLEAVED lane map (lane_map.h:
the two lane groups of a 16-lane DPP row on alternating lanes, each lane hand-over one row_shr:2).  Conventions as in
tests/test_gpu_sym_affine_side_tile.py: half-float cells off, the tile forced, every score compared EXACTLY with
oracle.cpu_ref.score(..., affine=True), and describe() says that the tile ran and in which form (ran_score_sym_affine_form).
The shapes are the smallest the map can go wrong at; tests/test_lane_map.py checks the map itself without a GPU.

  a. reads of 133 and 152 bases (the tile's window: a padding lane on top, none) x references of 1, 19, 20 and 41 bases (less
     than one trip of K = 19 steps, exactly one, one and a remainder, two and a remainder) x batches of 1, 2, 15, 16, 17 and 33
     pairs.  Every pair of a wave is different and -- where the reference has the columns for it -- has a score of its own, so a
     group or a half of the wave that is swapped, doubled or dropped shows at its own index; the odd counts end in a lone pair A,
     and the scores are stored through a pointer that is no multiple of 4 as well (the store of a lane's two scores one by one);
  b. a planted alignment whose vertical gap crosses each of the seven lane boundaries in turn (rows 19 k - 1 | 19 k): F of the
     lane below arrives through the hand-over or not at all; one alignment that starts in row 0, column 0 (the moving border of
     the group's first lane); one whose whole score lies in the last lane's rows (the result leaves through the reduction over
     the group, whose distances are the map's);
  c. the repairing form on the same shapes: an N before the last ACGT base of one reference in every wave."""
import numpy as np
import pytest

from oracle import cpu_ref
from test_gpu_sym_affine_max3 import _args, _device
from test_gpu_sym_affine_side_tile import ACCEPTED, _engine, _forced, _ran_tile
from test_sym_affine_row_tables_sweep import needs_repair
from versalignlib_amd import host

pytestmark = pytest.mark.gpu

G, K, ROWS = 8, 19, 152
READS = (133, 152)
COLUMNS = (1, 19, 20, 41)
PAIRS = (1, 2, 15, 16, 17, 33)
MATCH = ACCEPTED[0]
T = ord("T")
ACG = np.frombuffer(b"ACG", dtype=np.uint8)


def _oracle(reads, refs):
    return cpu_ref.score(host.SW, reads, refs, cpu_ref.Scoring.make(*_args(ACCEPTED)), threads=4, affine=True)


def _matches(i, F):
    """matching bases planted for pair i: one count per pair of a wave where the reference is long enough for 16 counts"""
    if F >= 19:
        return 3 + i % 16
    return bin(i).count("1") % 2          # F = 1: a match or none, in an order no swap of groups or halves keeps


def _batch(R, F, n, dirty=False):
    """References of A, C and G, reads of T but for the first _matches(i, F) reference bases planted at a row of their own:
    pair i scores exactly MATCH * _matches(i, F).  dirty: the first pair of every wave has an N in column 1, before its last base."""
    rng = np.random.default_rng(1000 * R + F)
    refs = np.ascontiguousarray(ACG[rng.integers(0, 3, size=(n, F))])
    reads = np.full((n, R), T, dtype=np.uint8)
    for i in range(n):
        m = _matches(i, F)
        at = (37 * i + 11) % (R - m + 1)
        reads[i, at:at + m] = refs[i, :m]
        if dirty and i % 16 == 0 and F > 2:
            refs[i, 1] = ord("N")
            assert needs_repair(refs[i])
    return reads, refs, {}


@pytest.mark.parametrize("F", COLUMNS)
@pytest.mark.parametrize("R", READS)
def test_every_group_and_half_of_a_wave_keeps_its_own_score(R, F):
    assert (F + G - 1 - (ROWS - R) // K) // K == {1: 0, 19: 1, 20: 1, 41: 2}[F]            # whole trips of the sweep: steps = F + G - 1 - lead
    batch = _batch(R, F, max(PAIRS))
    reads, refs, _ = batch
    exp = _oracle(reads, refs)
    assert exp.tolist() == [MATCH * _matches(i, F) for i in range(max(PAIRS))]             # by construction
    assert len({(r.tobytes(), f.tobytes()) for r, f in zip(reads, refs)}) == max(PAIRS) or F == 1
    for wave in range(0, max(PAIRS), 16):
        if F >= 19:
            assert len(set(exp[wave:wave + 16].tolist())) == len(exp[wave:wave + 16])
        else:
            assert exp[wave:wave + 8].tolist() != exp[wave + 8:wave + 16].tolist() and set(exp[:16].tolist()) == {0, MATCH}     # the halves differ
    batch[2][(ACCEPTED, host.SW)] = exp
    assert _forced(R, F, ACCEPTED, batch, PAIRS, form="row_tables") == ["row_tables"] * len(PAIRS)
    # ... and through a score pointer that is no multiple of 4: a lane stores its two scores one by one
    import torch
    eng = _engine(R, F, ACCEPTED)
    for n in (17, 33):
        out = torch.full((n + 1,), -7, dtype=torch.int16, device="cuda")
        assert out[1:].data_ptr() % 4 == 2
        eng.score_device(host.SW, _device(reads[:n].copy()), _device(refs[:n].copy()), scores=out[1:])
        got = out.cpu().numpy()
        _ran_tile(eng.describe(host.SW, n), (R, F, n, "unaligned scores"))
        assert got[0] == -7 and np.array_equal(got[1:], exp[:n]), (R, F, n, np.nonzero(got[1:] != exp[:n])[0][:8].tolist())
    eng.close()


@pytest.mark.parametrize("F", COLUMNS)
@pytest.mark.parametrize("R", READS)
def test_the_repairing_form_on_the_same_shapes(R, F):
    batch = _batch(R, F, max(PAIRS), dirty=True)
    exp = _oracle(batch[0], batch[1])
    assert exp.max() > 0
    batch[2][(ACCEPTED, host.SW)] = exp
    # (a reference of one base has no base before its last: nothing to repair, and the kernel says so)
    form = "row_tables_repair" if F > 2 else "row_tables"
    assert any(needs_repair(f) for f in batch[1]) == (F > 2)
    assert _forced(R, F, ACCEPTED, batch, PAIRS, form=form) == [form] * len(PAIRS)


# ---- b. planted alignments ----
def _planted(R, F):
    """16 constructions, one wave; -> reads, refs, the score each has by construction (None: see the oracle), what each is"""
    rng = np.random.default_rng(R + F)
    top = ROWS - R                                   # padded row of read position 0
    pairs = []

    def fresh():
        return np.full(R, T, dtype=np.uint8), np.ascontiguousarray(ACG[rng.integers(0, 3, size=F)])

    # a vertical gap of 2 and of 3 rows across each lane boundary: `a` reference bases end in padded row 19 k - 2, the gap's
    # rows hold T (no reference base: they match nothing), the next `b` reference bases follow below
    for k in range(1, G):
        for gap in (2, 3):
            read, ref = fresh()
            first_gap_row = K * k - 1
            a = min(20, first_gap_row - top)
            if a < 8:                                # (133 bases: the boundary 18 | 19 lies in the padding lane)
                continue
            r0 = first_gap_row - a - top             # read position of the first planted base
            b = min(20, R - (r0 + a + gap))          # (the last boundary: 17 or 18 rows are left below the gap)
            read[r0:r0 + a] = ref[:a]
            read[r0 + a + gap:r0 + a + gap + b] = ref[a:a + b]
            assert r0 >= 0 and r0 + a + gap + b <= R and a + b <= F
            # the gap's rows are the last of lane k - 1 and the first of lane k (and the second, for three rows)
            assert (top + r0 + a) // K == k - 1 and (top + r0 + a + 1) // K == k
            pairs.append((read, ref, ("gap", k, gap, a, b)))
    # starts in row 0, column 0 (of the read: with 133 bases that is lane 1's first row, whose diagonal is the padding lane's hand-over)
    read, ref = fresh()
    read[:17] = ref[:17]
    pairs.append((read, ref, ("origin", 17)))
    # the whole score inside the last lane's rows, at the reference's end
    read, ref = fresh()
    read[R - 15:R - 2] = ref[F - 13:]
    assert (top + R - 15) // K == G - 1
    pairs.append((read, ref, ("last-lane", 13)))
    return pairs


@pytest.mark.parametrize("R", READS)
def test_planted_alignments_cross_every_lane_boundary(R):
    F = 41
    pairs = _planted(R, F)
    assert len(pairs) == {152: 16, 133: 14}[R]
    assert {p[2][1] for p in pairs if p[2][0] == "gap"} == set(range(1 if R == 152 else 2, G))
    # a second wave holds the same constructions rotated by five places: each one in another group and the other half
    order = list(range(len(pairs))) + [(i + 5) % len(pairs) for i in range(len(pairs))]
    reads = np.ascontiguousarray(np.stack([pairs[i][0] for i in order]))
    refs = np.ascontiguousarray(np.stack([pairs[i][1] for i in order]))
    exp = _oracle(reads, refs)
    for at, i in enumerate(order):
        what = pairs[i][2]
        if what[0] == "gap":
            _, k, gap, a, b = what
            # both pieces and the gap between them: more than either piece alone can score, so the path crosses rows 19 k - 1 | 19 k
            # in a vertical gap (open -5, extend -1: 5 + (gap - 1) below the matches)
            assert exp[at] == MATCH * (a + b) - (5 + gap - 1) and exp[at] > MATCH * max(a, b), (what, exp[at])
        else:
            assert exp[at] == MATCH * what[1], (what, exp[at])
    batch = (reads, refs, {(ACCEPTED, host.SW): exp})
    n = len(order)
    assert _forced(R, F, ACCEPTED, batch, (n, len(pairs), 1), form="row_tables") == ["row_tables"] * 3
