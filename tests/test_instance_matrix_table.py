"""The instance matrix (tests/instance_matrix.py, walked on the GPU by tests/test_gpu_instance_matrix.py and
tests/test_gpu_placed_matrix.py) knows every geometry kernel_instances.hip.h compiles: a geometry added there fails here until it
joins the matrix.  The placed family's tables are held against the lookup functions of placed_kernels.hip.h and
extend_kernels.hip.h and against the key's constants in cell_rules.h, and the placed matrix's inputs
(tests/placed_matrix_cases.py) against the conditions that make its runs mean something."""
import os
import re

import pytest

import instance_matrix as im
import placed_matrix_cases as pm

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "versalignlib_amd", "csrc")
HEADER = os.path.join(CSRC, "kernel_instances.hip.h")


def _parsed():
    text = open(HEADER).read()
    parts = re.findall(r"^#define\s+VALIGN_PART(\d+)\(X, Y\)(.*)$", text, flags=re.M)
    table = {}
    for _, body in parts:
        for kind, G, K in re.findall(r"\b([XY])\((\d+),\s*(\d+)\)", body):
            assert (int(G), int(K)) not in table, ("listed twice", G, K)
            table[(int(G), int(K))] = kind == "X"
    return [int(p) for p, _ in parts], table


def test_matrix_lists_every_compiled_geometry():
    parts, table = _parsed()
    assert parts == list(range(6)), parts
    assert int(re.search(r"#define\s+VALIGN_KERNEL_PARTS\s+(\d+)", open(HEADER).read()).group(1)) == len(parts)
    assert table == im.GEOMETRIES


def test_instance_counts():
    full = sum(im.GEOMETRIES.values())
    fast = len(im.GEOMETRIES) - full
    assert (len(im.GEOMETRIES), full, fast) == (17, 6, 11)
    assert len(im.SCORE_INSTANCES) == 14 and len(im.FAST_FILLS) == 5 and len(im.FALLBACK_FILLS) == 16
    assert not im.FAST_FILLS & im.FALLBACK_FILLS
    assert 17 * 14 + 11 * 5 + 6 * 21 == 419
    assert sum(len(im.SCORE_INSTANCES) + len(im.carried_fills(G, K)) for G, K in im.GEOMETRIES) == 419
    # what the matrix proves launched: every score instance, and every fill instance but the two unselectable ones
    assert set(im.UNSELECTABLE) <= set(im.GEOMETRIES) and im.NEEDS_NO_TAG <= set(im.GEOMETRIES)
    assert all(im.UNSELECTABLE[g] <= im.carried_fills(*g) for g in im.UNSELECTABLE)
    assert sum(len(im.carried_fills(G, K) - im.UNSELECTABLE.get((G, K), frozenset())) for G, K in im.GEOMETRIES) == 179


def test_header_macros_list_the_carried_kernels():
    """VALIGN_FAST_KERNELS / VALIGN_FALLBACK_KERNELS hold as many instances as the matrix expects of a geometry."""
    text = open(HEADER).read()
    fast = text[text.index("#define VALIGN_FAST_KERNELS"):text.index("#define VALIGN_FALLBACK_KERNELS")]
    fallback = text[text.index("#define VALIGN_FALLBACK_KERNELS"):text.index("#define VALIGN_PLACED_KERNELS")]
    assert len(re.findall(r"PREFIX __global__ void score_kernel<", fast)) == len(im.SCORE_INSTANCES)
    assert len(re.findall(r"PREFIX __global__ void align_fill\w*<", fast)) == len(im.FAST_FILLS)
    assert len(re.findall(r"PREFIX __global__ void align_fill\w*<", fallback)) == len(im.FALLBACK_FILLS)
    assert "score_kernel<" not in fallback


def test_shapes_and_batch():
    for (G, K) in im.GEOMETRIES:
        ppw = 2 * (64 // G)
        n = im.batch(G)
        assert n == 4 * ppw + ppw // 2 + 1         # a full four-wave block and a second, partly filled one
        assert G == 64 or ((n - 4 * ppw) < ppw and (n - 4 * ppw) % 2 == 1)      # (two pairs per wave: the extra wave is whole)
        for R, F in im.shapes(G, K):
            assert 0 < R <= G * K and F > 0 and R + F <= 32767
        assert {R for R, _ in im.shapes(G, K)} == {G * K, G * K - K - 1}
        assert all(F % 4 != 0 for _, F in im.shapes(G, K) if F == 2 * G + 7)
    assert len(im.SCORINGS) == 20 and len(set(im.SCORINGS)) == 20


# ---- the placed family ----
def test_placed_instance_counts():
    geoms = sorted(im.GEOMETRIES)
    placed = {g: im.carried_placed(*g) for g in geoms}
    assert sum(len(v) for v in placed.values()) == 68
    assert sum(len(im.carried_subopt(*g)) for g in geoms) == 44
    assert sum(len(im.carried_extend(*g)) for g in geoms) == 24
    # key track, Sym / AffineSym, on the 15 geometries with K <= 16; key track, Linear / Affine, on the five full ones among
    # them; rows track, all four forms, on the six full geometries and 64 x 24
    key_sym = [(g, i) for g in geoms for i in placed[g] if i[0] == "key" and i[1] in im.PLACED_SYM_FORMS]
    key_asym = [(g, i) for g in geoms for i in placed[g] if i[0] == "key" and i[1] not in im.PLACED_SYM_FORMS]
    rows = [(g, i) for g in geoms for i in placed[g] if i[0] == "rows"]
    assert (len(key_sym), len(key_asym), len(rows)) == (30, 10, 28)
    assert {g for g, _ in key_sym} == {g for g in geoms if g[1] <= 16} and len({g for g, _ in key_sym}) == 15
    assert {g for g, _ in key_asym} == {g for g in geoms if g[1] <= 16 and im.GEOMETRIES[g]} and len({g for g, _ in key_asym}) == 5
    assert {g for g, _ in rows} == {g for g in geoms if im.GEOMETRIES[g]} | {(64, 24)} and len({g for g, _ in rows}) == 7
    for g in geoms:
        assert im.carried_subopt(*g) <= placed[g] and im.carried_extend(*g) <= placed[g]
        assert all(t in pm.TRACKS and f in im.PLACED_FORMS for t, f in placed[g])
        assert set(im.PLACED_UNSELECTABLE.get(g, {})) <= placed[g]
    assert set(im.PLACED_UNSELECTABLE) <= set(geoms)
    assert set(pm.FORM_NAMES.values()) == set(im.PLACED_FORMS) and set(pm.FORM_NAMES) == set(pm.FORMS)


def _lookup_body(text, name):
    """the lines of a lookup function that fill its table: from behind the table's declaration to the function's return"""
    at = text.index("\n", text.index("const void *%s[" % name))
    return text[at:text.index("return", at)]


def test_lookup_functions_assign_the_carried_instances():
    """placed_kernel / subopt_kernel / extend_kernel hold one table assignment per distinct (track, form) of the matrix"""
    placed_h = open(os.path.join(CSRC, "placed_kernels.hip.h")).read()
    extend_h = open(os.path.join(CSRC, "extend_kernels.hip.h")).read()
    distinct = lambda carried: set().union(*(carried(*g) for g in im.GEOMETRIES))
    placed = re.findall(r"^\s*placed\[(\w+)\]\[(\w+)\] = \(const void \*\)&score_placed_kernel<G, K, (\w+), (\w+)>;", _lookup_body(placed_h, "placed"), flags=re.M)
    sub = re.findall(r"^\s*sub\[(\w+)\]\[(\w+)\] = \(const void \*\)&score_placed_kernel<G, K, (\w+), (\w+), true>;", _lookup_body(placed_h, "sub"), flags=re.M)
    ext = re.findall(r"^\s*ext\[(\w+)\] = \(const void \*\)&score_extend_kernel<G, K, (\w+)>;", _lookup_body(extend_h, "ext"), flags=re.M)
    assert len(placed) == len(distinct(im.carried_placed)) == 8 and len(set(placed)) == 8
    assert len(sub) == len(distinct(im.carried_subopt)) == 8 and len(set(sub)) == 8
    assert len(ext) == len(distinct(im.carried_extend)) == 4 and len(set(ext)) == 4
    # every slot holds the instance of its own indices
    assert all((track, gaps) == (t2, g2) for track, gaps, g2, t2 in placed + sub) and all(a == b for a, b in ext)
    names = {"kPlacedKey": "key", "kPlacedRows": "rows", "kGapLinear": "Linear", "kGapSym": "Sym", "kGapAffine": "Affine", "kGapAffineSym": "AffineSym"}
    assert {(names[t], names[g]) for t, g, _, _ in placed} == distinct(im.carried_placed)
    assert {(names[t], names[g]) for t, g, _, _ in sub} == distinct(im.carried_subopt)
    assert {("rows", names[g]) for g, _ in ext} == distinct(im.carried_extend)
    assert len(re.findall(r"\[\w+\]\s*=[^=]", _lookup_body(placed_h, "placed"))) == 8         # (no assignment line the patterns above missed)
    assert len(re.findall(r"\[\w+\]\s*=[^=]", _lookup_body(placed_h, "sub"))) == 8
    assert len(re.findall(r"\[\w+\]\s*=[^=]", _lookup_body(extend_h, "ext"))) == 4


def test_key_constants_of_cell_rules():
    """kPlacedKeyMaxK and placed_key_bits as cell_rules.h states them: 16, and 2 / 3 / 4 bits by K -- what the matrix, and the
    restated rules of the GPU tests, count on"""
    text = open(os.path.join(CSRC, "cell_rules.h")).read()
    assert int(re.search(r"constexpr int kPlacedKeyMaxK = (\d+);", text).group(1)) == 16 == im.PLACED_KEY_MAX_K
    m = re.search(r"constexpr int placed_key_bits\(int K\) \{ return K <= (\d+) \? (\d+) : \(K <= (\d+) \? (\d+) : (\d+)\); \}", text)
    assert m, "placed_key_bits is no longer the two-threshold expression this test reads"
    k1, b1, k2, b2, b3 = (int(v) for v in m.groups())
    assert (k1, b1, k2, b2, b3) == (4, 2, 8, 3, 4)
    for K in range(1, 33):
        assert im.placed_key_bits(K) == (b1 if K <= k1 else (b2 if K <= k2 else b3))
    # every row of a lane has a code of its own below the value
    assert all((1 << im.placed_key_bits(K)) >= K for _, K in im.GEOMETRIES if K <= 16)
    assert re.search(r"if \(K <= kPlacedKeyMaxK && \(\(top \+ 1\) << bits\) <= 32000\)", text)


def test_placed_matrix_scorings():
    for G, K, R, F in pm.CASES:
        assert min(R, F) <= 135
        for track in pm.tracks(K):
            for form in pm.FORMS:
                args = pm.scoring_args(track, form, R, F, K)
                top = min(R, F) * args[0]
                inside = ((top + 1) << im.placed_key_bits(K)) <= 32000
                assert inside == (track == "key") and top + 1 <= 32000 and args[1] < 0, (G, K, R, F, track, form, args)
        assert ("key" in pm.tracks(K)) == (K <= 16)
    assert len(pm.CASES) == 68 and sum(len(pm.tracks(K)) * len(pm.FORMS) for _, K, _, _ in pm.CASES) == 512


@pytest.mark.parametrize("geom", sorted(im.GEOMETRIES), ids=lambda g: "%dx%d" % g)
def test_placed_matrix_inputs(geom):
    """Every run of the placed matrix on this geometry: the batch has both kinds of pairs, and the reference alone says that the
    random ones score, end in more than one lane and include a read trimmed by more than a lane, and that the planted ties'
    records are the construction's (placed_matrix_cases.input_problems)."""
    G, K = geom
    for R, F in im.shapes(G, K):
        reads, refs, random_at, where = pm.batch(G, K, R, F)
        n = im.batch(G)
        assert reads.shape == (n, R) and refs.shape == (n, F) and len(random_at) + len(where) == n
        assert len(where) >= pm.MIN_PLANTED and len(random_at) >= len(where) and (G == 64 or len(random_at) >= 2 * len(where))
        pad = G * K - R
        tie_lanes = [((r - 1 + pad) // K) for r, _ in where.values()]
        assert len(set(tie_lanes)) >= 3 and min(tie_lanes) == (pad // K) and {c for _, c in where.values()} >= {F}
        for track in pm.tracks(K):
            for form in pm.FORMS:
                problems = pm.input_problems(G, K, R, F, track, form)
                assert not problems, (G, K, R, F, track, form, problems[:3])
