"""The table behind tests/test_gpu_instance_matrix.py and tests/test_gpu_placed_matrix.py: every (G, K) register geometry
libHIPKernel.so is compiled for, the kernel instances each one carries (kernel_instances.hip.h; placed_kernels.hip.h and
extend_kernels.hip.h for the placed family), and the shapes, batch and scorings that reach them through the public API.  No GPU
here: tests/test_instance_matrix_table.py checks this table against the headers."""

# (group lanes, rows per lane) -> full: the geometry carries the fallback fill kernels too
GEOMETRIES = {
    (8, 4): False, (8, 6): False, (8, 8): True, (16, 4): False, (8, 10): False, (8, 12): False, (16, 8): False,
    (16, 10): True, (16, 12): False, (32, 8): False, (32, 10): True, (32, 12): False, (64, 8): True, (64, 12): False,
    (64, 16): True, (64, 24): False, (64, 32): True,
}

# score_kernel<G, K, ALG, GAPS>: seven gap forms for each algorithm, on every geometry
SCORE_FORMS = ("Linear", "Sym", "Affine", "AffineSym", "AffineSymF16", "AffineF16", "SymF16")
SCORE_INSTANCES = frozenset((alg, form) for alg in ("SW", "NW") for form in SCORE_FORMS)

# fill kernels by describe()'s ran_align_fill: VALIGN_FAST_KERNELS on every geometry, VALIGN_FALLBACK_KERNELS on the full ones
FAST_FILLS = frozenset({("SW", "tag_key"), ("SW", "tag_prof_key"), ("SW", "affine_tag_sym"), ("NW", "tag"), ("NW", "affine_tag_sym")})
FALLBACK_FILLS = frozenset(
    {("SW", f) for f in ("linear", "linear_sym", "affine", "affine_sym", "sse", "tag", "sse_tag", "sse_tag_key", "affine_tag")} |
    {("NW", f) for f in ("linear", "linear_sym", "affine", "affine_sym", "sse", "sse_tag", "affine_tag")})

# The ONLY instances the matrix may leave unreached: compiled, but no call can select them -- the key rides in the query
# profile only where 64x the cell range fits, which prof_key_ok (cell_rules.h) grants for K <= 16.
UNSELECTABLE = {(64, 24): frozenset({("SW", "tag_prof_key")}), (64, 32): frozenset({("SW", "tag_prof_key")})}

# Geometries on which no scoring of the pool reaches a carried kernel at the matrix's shapes without the debug switch
# no_tag: NW linear_sym on 64 x 32 (every symmetric linear scoring of the pool that stays on the register path at 2 048 rows is
# inside the tagged cells' range, so the tagged NW kernel takes it)
NEEDS_NO_TAG = {(64, 32)}


def carried_fills(G, K):
    return FAST_FILLS | (FALLBACK_FILLS if GEOMETRIES[(G, K)] else frozenset())


# ---- the placed family: score_placed_kernel<G, K, GAPS, TRACK[, SUB]> and score_extend_kernel<G, K, GAPS>, looked up by
# placed_kernel / subopt_kernel (placed_kernels.hip.h) and extend_kernel (extend_kernels.hip.h); walked on the GPU by
# tests/test_gpu_placed_matrix.py.  An instance is (track, form): track as describe()'s ran_placed names it ----
PLACED_FORMS = ("Linear", "Sym", "Affine", "AffineSym")
PLACED_SYM_FORMS = ("Sym", "AffineSym")
PLACED_KEY_MAX_K = 16           # kPlacedKeyMaxK (cell_rules.h): the lane key exists for up to 16 rows per lane


def placed_key_bits(K):
    """placed_key_bits (cell_rules.h): the bits of the row below the value in the lane key"""
    return 2 if K <= 4 else (3 if K <= 8 else 4)


def carried_placed(G, K):
    """The key track with the symmetric forms wherever the key exists, with all four on the full geometries; the rows track with
    all four on the full geometries and on 64 x 24."""
    full = GEOMETRIES[(G, K)]
    out = set()
    if K <= PLACED_KEY_MAX_K:
        out |= {("key", f) for f in (PLACED_FORMS if full else PLACED_SYM_FORMS)}
    if full or (G, K) == (64, 24):
        out |= {("rows", f) for f in PLACED_FORMS}
    return frozenset(out)


def carried_subopt(G, K):
    """The suboptimal form of the placed sweep: the full geometries only, the key track where the key exists."""
    if not GEOMETRIES[(G, K)]:
        return frozenset()
    return frozenset((t, f) for t in (("key", "rows") if K <= PLACED_KEY_MAX_K else ("rows",)) for f in PLACED_FORMS)


def carried_extend(G, K):
    """Extension scores: the rows track's sweep, on the full geometries only."""
    return frozenset(("rows", f) for f in PLACED_FORMS) if GEOMETRIES[(G, K)] else frozenset()


# Placed instances the matrix cannot select at its shapes, as {(G, K): {(track, form): reason}}: none -- min(R, F) <= 135 there,
# so match 2 is inside the key's range at every K <= 16, and a match beyond it stays inside int16.
PLACED_UNSELECTABLE = {}


def shapes(G, K):
    """R = G K: every register row is real; R = G K - K - 1: one lane all padding, the next partly (the SW sweep starts at a
    later lane).  F = G / 2 + 3: fill and drain overlap; F = 2 G + 7: fill, steady state and drain, odd step count, F % 4 != 0."""
    return [(R, F) for R in (G * K, G * K - K - 1) for F in (G // 2 + 3, 2 * G + 7)]


def batch(G):
    """One full four-wave block plus a partial wave with an odd pair count (G = 64, two pairs per wave: plus one whole wave)."""
    ppw = 2 * (64 // G)
    return 4 * ppw + ppw // 2 + 1


# Arguments of Scoring.make: match, mismatch, gap_read, gap_ref[, open_read, ext_read, open_ref, ext_ref]
LINEAR = [(1, -1, -1, -1), (1, -1, -1, -2), (2, -1, -3, -3), (2, -1, -2, -4), (14, -11, -20, -20), (14, -11, -20, -18),
          (60, -40, -50, -50), (60, -40, -50, -45), (400, -300, -350, -350), (400, -300, -350, -340)]
AFFINE = [(m, x, -3, -3) + g for m, x, pair in (
    (1, -1, ((-2, -1, -2, -1), (-2, -1, -3, -1))),
    (2, -1, ((-5, -1, -5, -1), (-5, -1, -4, -2))),
    (14, -11, ((-20, -3, -20, -3), (-20, -3, -18, -3))),
    (60, -40, ((-50, -10, -50, -10), (-50, -10, -45, -10))),
    (400, -300, ((-350, -100, -350, -100), (-350, -100, -340, -100)))) for g in pair]
SCORINGS = LINEAR + AFFINE
