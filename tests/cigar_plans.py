"""Alignments planted run by run, for the lane-group CIGAR encoders (cigar_encode_kernel / span_cigar_encode_kernel<16 | 64>).
Pure Python and numpy: nothing of the library, nothing of the oracle.

A plan is a list of (length, op), op one of "=", "X", "I", "D" (I: read bases against a gap in the reference, D: reference bases
against a gap in the read).  build(plan, R, F, rng) returns ONE NUL-padded read and reference that begin at column 0 and whose
Smith-Waterman alignment, under either scoring of SCORINGS, is the plan and nothing else.  tests/test_cigar_plans.py holds
every plan of plans(W) to that on the oracle (cpu_ref.align under both tie-break policies, and the alignment of the reversed
pair); the GPU tests (tests/test_gpu_cigar_plans.py) then know every run boundary of every alignment they hand to the encoder.

The two scorings: match 5, mismatch -1 and either linear gaps of -12 a base ("lin") or affine gaps of -12 to open (the first gap
base) and -1 to extend ("aff").  A gap run costs at least 12 and a mismatch 1, and a gap run in the read needs one in the
reference to make up for it before the bases line up again, so no gap replaces a mismatch; a match is worth 5, so a flank of k
matches outweighs what costs less than 5 k between two flanks.

What build() does about ambiguity (it refuses a plan it cannot make unique, it does not hope):
  * no two neighbouring bases of the read are equal, nor of the reference: no run of one letter in which a gap could slide;
  * a gap run's first base differs from the base that follows the run, and its last base from the base in front of the run (on the
    other sequence these are the same bases: the flanks are "=" columns): the run cannot shift by one column, or by k, at no
    cost -- a shift to the left by k aligns the run's last base with the base in front of it, a mismatch in place of a match;
  * under linear gaps a run also SPLITS at no cost (a flank base may sit anywhere inside it), so in a plan made for the linear
    scoring no base of a gap run of two or more equals the base in front of the run or the base behind it: the run alternates
    between two letters, and the base behind is the third letter that is not the base in front;
  * the two bases of an "X" column differ;
  * the bases of an "X" column and of the column behind it also differ, wherever four letters allow it after the rules above,
    from the base two places back on either sequence: the alignment shifted by two columns finds no match there (without
    this "=X=X=X ..." is beaten by its own shift: an "=" base has two letters to choose from, one of them the "=" base two
    columns back).  Only there: every letter that is ruled out makes the letters that remain likelier, so as a rule for every
    column it would make a base equal the base three back every other time, and a shift by three would win;
  * a plan begins and ends with an "=" run; gap runs and "X" runs stand between "=" runs, and build() asserts that each such
    flank outweighs the run AND what unrelated bases gain by chance: neighbouring-distinct random bases match one time in
    three at most, a column of them gains 5 / 3 - 2 / 3 = 1 on average, so an alignment that leaves a flank of k columns for
    another diagonal gains about k there and loses 5 k; build() asks for 5 k - cost > 2 k, twice the expectation, and of a
    flank between two such runs that it outweighs both together (an I run, a short flank and a D run are otherwise traded
    for one short gap and a flank of chance);
  * "X" runs are at most MAX_X_RUN columns: a long run of mismatches between random bases is beaten by a shifted alignment of
    the same bases (one gap at either end, a quarter of the columns then match), whatever the flanks.
What remains is chance on far diagonals, against margins of that size; the pairs come from fixed seeds, and
tests/test_cigar_plans.py holds every one of them to the oracle.

An "I" run directly followed by a "D" run (or the other way round) is NOT among the plans: neither scoring admits one.  k read
bases against k reference bases as "X" columns cost at most k; as an I run and a D run they cost at least 24.  Every optimal
alignment therefore has at least one "=" or "X" column between two gap runs of different kinds; plans() has I = D with a short
flank between them instead.

Lowercase bases (either side) and N / N columns: an "=" column whose read base is lowercase is still "=" and still scores a
match; a column of two N is "=" by the column rule (the bytes are equal) and adds nothing to the score.
"""
import collections
import random

import numpy as np

MATCH, MISMATCH = 5, -1
GAP = -12                      # linear: every gap base
OPEN, EXT = -12, -1            # affine: the first base of a gap run, every further one
SCORINGS = {"lin": (MATCH, MISMATCH, GAP, GAP), "aff": (MATCH, MISMATCH, GAP, GAP, OPEN, EXT, OPEN, EXT)}
MAX_X_RUN = 2
LINEAR_GAP_MAX = 8             # gap runs of the plans made for the linear scoring
BASES = "ACGT"

M, I, D, EQ, X = 0, 1, 2, 7, 8           # BAM codes of the compact result format
CODE = {"=": EQ, "X": X, "I": I, "D": D}

# name ..... unique within plans(W)
# pins ..... the statement of cigar_encode_kernel (and of its backward twin) the case is there for
# runs ..... the plan; empty for the two empty alignments (kind "noshare": no base of the read occurs in the reference, "nul": a
#            read of NULs only)
# forms .... the scorings it is made for
# lower_read / lower_ref / n_at: columns whose read / reference base is lowercase, columns of N / N (all inside "=" runs)
Case = collections.namedtuple("Case", "name pins runs forms lower_read lower_ref n_at kind")


def is_affine(form):
    return form == "aff"


def scoring(form, make):
    """make: cpu_ref.Scoring.make or hipkernel.Scoring.make"""
    return make(*SCORINGS[form])


def run_cost(length, op, form):
    """what a run takes from the score (>= 0); "=" runs cost nothing"""
    if op == "X":
        return -MISMATCH * length
    if op in "ID":
        return -GAP * length if form == "lin" else -(OPEN + EXT * (length - 1))
    return 0


def columns(runs):
    return sum(length for length, _ in runs)


def read_bases(runs):
    return sum(length for length, op in runs if op != "D")


def ref_bases(runs):
    return sum(length for length, op in runs if op != "I")


def score(case, form):
    """the plan's score by construction"""
    gained = MATCH * (sum(length for length, op in case.runs if op == "=") - len(case.n_at))
    return gained - sum(run_cost(length, op, form) for length, op in case.runs)


def ops(runs, extended=True):
    """the plan as ops of the compact result format (length << 4 | code); not extended: "=" and "X" merge into M"""
    out = []
    for length, op in runs:
        code = CODE[op] if extended or op in "ID" else M
        if out and out[-1][1] == code:
            out[-1][0] += length
        else:
            out.append([length, code])
    return [(length << 4) | code for length, code in out]


def record(case, form, extended=True):
    """(read_begin, read_end, ref_begin, ref_end, score, n_ops) by construction; all zeros for an empty alignment"""
    if not case.runs:
        return (0, 0, 0, 0, 0, 0)
    return (0, read_bases(case.runs), 0, ref_bases(case.runs), score(case, form), len(ops(case.runs, extended)))


def boundaries(runs, extended=True):
    """the columns at which a run begins -- the lanes whose `boundary` is set -- column 0 included"""
    out, at, prev = [], 0, None
    for length, op in runs:
        code = CODE[op] if extended or op in "ID" else M
        if code != prev:
            out.append(at)
        prev = code
        at += length
    return out


def _check_plan(runs, forms):
    assert runs and runs[0][1] == "=" and runs[-1][1] == "=", "a plan begins and ends with an '=' run"
    for k, (length, op) in enumerate(runs):
        assert length >= 1 and op in CODE, (length, op)
        if k:
            assert runs[k - 1][1] != op, "neighbouring runs of one op are one run"
        if op == "=":
            continue
        assert runs[k - 1][1] == "=" and runs[k + 1][1] == "=", "gap runs and X runs stand between '=' runs"
        assert op != "X" or length <= MAX_X_RUN, "a long X run is not unique (module docstring)"
        cost = max(run_cost(length, op, f) for f in forms)
        assert (MATCH - 2) * min(runs[k - 1][0], runs[k + 1][0]) > cost, ("a flank does not outweigh its neighbour", runs[k - 1:k + 2])
        if k + 2 < len(runs) - 1:     # a flank between two runs outweighs both: an alignment may leave it to trade them for one
            both = cost + max(run_cost(runs[k + 2][0], runs[k + 2][1], f) for f in forms)
            assert (MATCH - 2) * runs[k + 1][0] > both, ("a flank does not outweigh its two neighbours", runs[k:k + 3])


def _pick(rng, hard, soft=()):
    """a base outside `hard`, and outside `soft` as far as that leaves one (the last of `soft` is given up first)"""
    soft = list(soft)
    while True:
        left = [b for b in BASES if b not in hard and b not in soft]
        if left:
            return rng.choice(left)
        soft.pop()


def _back(seq, k):
    return seq[-k] if len(seq) >= k else ""


def build(plan, R, F, rng, lower_read=(), lower_ref=(), n_at=(), forms=("lin", "aff")):
    """-> read uint8 [R], ref uint8 [F], NUL-padded, whose alignment under the scorings `forms` is uniquely `plan`
    (module docstring).  rng: a random.Random."""
    _check_plan(plan, forms)
    assert read_bases(plan) <= R and ref_bases(plan) <= F, ("the plan does not fit", read_bases(plan), R, ref_bases(plan), F)
    read, ref = [], []                # upper case; "" in front of the first base
    col_of_read, col_of_ref = [], []
    avoid = ()                        # after a gap run: what the next column's base must not be (the run's first base)
    after_x = False                   # the column behind an X column
    col = 0
    for length, op in plan:
        if op == "=":
            for _ in range(length):
                if col in n_at:
                    b = "N"
                else:
                    b = _pick(rng, (_back(read, 1), _back(ref, 1)) + avoid, (_back(read, 2), _back(ref, 2)) if after_x else ())
                read.append(b)
                ref.append(b)
                col_of_read.append(col)
                col_of_ref.append(col)
                avoid, after_x = (), False
                col += 1
        elif op == "X":
            for _ in range(length):
                r = _pick(rng, (read[-1],), (_back(ref, 2), _back(read, 2)))
                f = _pick(rng, (ref[-1], r), (_back(read, 2), _back(ref, 2)))
                read.append(r)
                ref.append(f)
                col_of_read.append(col)
                col_of_ref.append(col)
                after_x = True
                col += 1
        else:
            seq, cols, other = (read, col_of_read, ref) if op == "I" else (ref, col_of_ref, read)
            front = other[-1]         # the base in front of the run (the same on both sequences: an "=" column)
            if "lin" in forms and length > 1:
                # linear gaps: a run splits at no cost, so NO base of the run may equal the base in front or the base behind.
                # The run alternates between two letters; the base behind is the third that is not the base in front.
                behind = _pick(rng, (front,))
                pair = [b for b in BASES if b not in (front, behind)]
                rng.shuffle(pair)
                for k in range(length):
                    seq.append(pair[k & 1])
                    cols.append(col)
                    col += 1
                avoid = tuple(b for b in BASES if b != behind)
                continue
            first = None
            for k in range(length):
                b = _pick(rng, (seq[-1], front if k == length - 1 else ""))
                first = first or b
                seq.append(b)
                cols.append(col)
                col += 1
            avoid = (first,)
    assert all(col_of_read[k] not in n_at or read[k] == "N" for k in range(len(read)))
    out_read, out_ref = np.zeros(R, np.uint8), np.zeros(F, np.uint8)
    for out, seq, cols, lower in ((out_read, read, col_of_read, set(lower_read)), (out_ref, ref, col_of_ref, set(lower_ref))):
        text = "".join(b.lower() if c in lower else b for b, c in zip(seq, cols))
        out[:len(text)] = np.frombuffer(text.encode(), np.uint8)
    return out_read, out_ref


def build_empty(kind, R, F):
    """the two empty alignments: "noshare" -- a read of A and C against a reference of G and T --, "nul" -- a read of NULs"""
    read, ref = np.zeros(R, np.uint8), np.zeros(F, np.uint8)
    ref[:] = np.frombuffer(b"GT" * F, np.uint8)[:F]
    if kind == "noshare":
        read[:] = np.frombuffer(b"AC" * R, np.uint8)[:R]
    else:
        assert kind == "nul", kind
    return read, ref


def _flank(cost):
    """'=' columns that outweigh `cost` and what chance gains elsewhere (module docstring), with a margin"""
    return cost // (MATCH - 2) + 6


def _start(first, W, cost):
    """the first column congruent to `first` modulo W whose '=' flank in front does the same"""
    while first < _flank(cost):
        first += W
    return first


def plans(W):
    """The cases of a lane width W (16 or 64), each with the statement of the encoder it pins."""
    assert W in (16, 64)
    out = []

    def add(name, pins, runs, forms=("lin", "aff"), lower_read=(), lower_ref=(), n_at=(), kind="plan"):
        out.append(Case(name, pins, tuple(runs), tuple(forms), tuple(lower_read), tuple(lower_ref), tuple(n_at), kind))

    tail = 12                          # the closing '=' flank behind a single X
    # ---- one '=' run of c columns ----
    add("eq1", "one lane valid (`valid = c < end`), the run opened on lane 0 and stored by the store behind the loop", [(1, "=")])
    add("eq%d" % (W - 1), "a partial only step: `carry_len = nvalid - last` with nvalid = W - 1", [(W - 1, "=")])
    add("eq%d" % W, "one whole step and no partial one: `steps = (cols + W - 1) / W`, carry_len = W", [(W, "=")])
    add("eq%d" % (W + 1), "a last step of one column without a boundary: `first = ... : nvalid` with nvalid = 1", [(W + 1, "=")])
    add("eq%d" % (2 * W), "a whole last step without a boundary: `carry_len += first` with first = nvalid = W", [(2 * W, "=")])
    add("eq%d" % (2 * W + 1), "the carry over a whole step and into a partial one, closed by the loop's end", [(2 * W + 1, "=")])
    add("eq%d" % (3 * W - 1), "a middle step with no boundary at all (`first = nvalid`, gm == 0: carry_op, count untouched)", [(3 * W - 1, "=")])
    # ---- every column a boundary ----
    add("alternate", "a ballot of all ones: `above = l == 63 ? 0 : gm >> (l + 1)` on the last lane, `count += popcll(gm)` = W a step, "
        "every run but a step's last closed inside the step with length ffsll(above) = 1", [(1, "="), (1, "X")] * (W + 1) + [(1, "=")])
    # ---- one X at column q ----
    for q in (W - 2, W - 1, W, W + 1, 2 * W - 1, 2 * W):
        lane = q % W
        what = {W - 2: "the X closed inside the step by the '=' on the last lane, which is carried on (`last`, `last_op = shfl(op, last)`)",
                W - 1: "a boundary on the last lane (`above` is 0 there: the X is carried, carry_len = 1) and one on lane 0 of the next step (first == 0)",
                0: "a boundary on lane 0: `prev = carry_op` decides it; the carried '=' run is closed with first == 0",
                1: "the carried run closed by `first` = 1: ffsll(gm) - 1 counts lane 0 into it"}[lane]
        add("x@%d" % q, what, [(q, "="), (1, "X"), (tail, "=")])
    add("x2@%d" % (W - 1), "an X run across the step edge: lane 0 is no boundary (`prev = carry_op` equals its op), carry_len = 1 + first",
        [(W - 1, "="), (2, "X"), (tail, "=")])
    # ---- a run from the last lane of a step across two whole steps to lane 0 of the fourth ----
    add("span2steps", "a run opened on the last lane, carried through two steps without a boundary (carry_len += W twice), closed on lane 0 of "
        "the fourth step: the stored length is 2 W + 1, its index count - 1", [(W - 2, "="), (1, "X"), (2 * W + 1, "="), (1, "X"), (tail, "=")])
    # ---- gap runs between '=' flanks ----
    for op in "ID":
        for length in sorted({1, 2, LINEAR_GAP_MAX, W - 1, W, 2 * W + 1}):
            forms = tuple(f for f in ("lin", "aff") if f == "aff" or length <= LINEAR_GAP_MAX)
            cost = max(run_cost(length, op, f) for f in forms)
            for lane in (W - 1, 0):
                q = _start(lane or W, W, cost)
                what = ("a %s run from the last lane on: lane 0 of the next step extends it (`prev == kCigar%s` with prev = carry_op), no boundary there"
                        % (op, op) if lane else "a %s run opened on lane 0 (`prev = carry_op` is the '=' run: the gap's opening score)" % op)
                if length == 1 and lane:
                    what = "a %s run of one column on the last lane: opened there, closed on lane 0" % op
                add("%s%d@%d" % (op, length, q), what, [(q, "="), (length, op), (_flank(cost), "=")], forms=forms)
    add("I=D", "both gap kinds in one alignment, a short '=' run between them: `prev == kCigarD` / `prev == kCigarI` each see the other op's "
        "neighbourhood", [(W - 3, "="), (2, "I"), (24, "="), (3, "D"), (W, "=")])
    # ---- lowercase and N ----
    add("case+N", "`(ca | 0x20) == (cb | 0x20)`: a lowercase base on one side is '=' (and scores a match: base_class), lowercase against another "
        "letter is X; N / N is '=' and scores nothing", [(W + 4, "="), (1, "X"), (tail, "=")], lower_read=(1, W - 1, W, W + 4), lower_ref=(2, W + 1),
        n_at=(W + 2,))
    # ---- the empty alignment ----
    add("noshare", "cols == 0: no step, no op, a record of zeros (`if (cols > 0)`)", [], kind="noshare")
    add("nul", "cols == 0 for a read of NULs", [], kind="nul")
    assert len({c.name for c in out}) == len(out)
    return out


def shape(W):
    """The shape the plans of W are run at: the engine's own choice of the width (256 x 400: 16, 257 x 400: 64)"""
    return (256, 400) if W == 16 else (257, 400)


STRIP_SHAPE = (1025, 1200)     # a read beyond the register geometries: the alignment runs on row strips


def strip_case():
    """The one long plan: 1025 columns (65 steps of 16, 17 of 64), '=' runs of 255, 447 and 321 columns and two X, both on a last
    lane of either width"""
    return Case("strip", "carry_len over many steps: a run of 447 columns is 27 steps of 16 without a boundary; an X on the last lane of a step",
                ((255, "="), (1, "X"), (447, "="), (1, "X"), (321, "=")), ("lin", "aff"), (), (), (), "plan")


def build_case(case, R, F, rng):
    if case.kind != "plan":
        return build_empty(case.kind, R, F)
    return build(case.runs, R, F, rng, case.lower_read, case.lower_ref, case.n_at, case.forms)


def batch(cases, R, F, seed=1):
    """-> reads uint8 [n, R], refs uint8 [n, F]: case k from a generator of its own (seed, k), so that a case's pair does not
    depend on its neighbours"""
    reads, refs = np.zeros((len(cases), R), np.uint8), np.zeros((len(cases), F), np.uint8)
    for k, case in enumerate(cases):
        reads[k], refs[k] = build_case(case, R, F, random.Random("%d/%s" % (seed, case.name)))
    return reads, refs


def for_form(cases, form):
    return [c for c in cases if form in c.forms]


def edges(cases, W):
    """Which of the encoder's edges the plans hold, computed from their boundaries (extended ops): a dict of sets of case names
      last_lane ..... a boundary at q % W == W - 1
      lane0 ......... a boundary at q > 0 with q % W == 0
      quiet_step .... a step (whole or partial, not the first) without a boundary
      full_step ..... a whole step of W boundaries
      carried_2 ..... a run that covers two whole steps without beginning or ending in them"""
    out = {k: set() for k in ("last_lane", "lane0", "quiet_step", "full_step", "carried_2")}
    for c in cases:
        if not c.runs:
            continue
        at = boundaries(c.runs)
        cols = columns(c.runs)
        per_step = collections.Counter(q // W for q in at)
        steps = (cols + W - 1) // W
        if any(q % W == W - 1 for q in at):
            out["last_lane"].add(c.name)
        if any(q and q % W == 0 for q in at):
            out["lane0"].add(c.name)
        quiet = [s for s in range(1, steps) if per_step[s] == 0]
        if quiet:
            out["quiet_step"].add(c.name)
        if any(per_step[s] == W for s in range(steps)):
            out["full_step"].add(c.name)
        if any(s + 1 in quiet and (s + 2) * W <= cols for s in quiet):
            out["carried_2"].add(c.name)
    return out
