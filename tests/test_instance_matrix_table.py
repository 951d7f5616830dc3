"""The instance matrix (tests/instance_matrix.py, walked on the GPU by tests/test_gpu_instance_matrix.py) knows every geometry
kernel_instances.hip.h compiles: a geometry added there fails here until it joins the matrix."""
import os
import re

import instance_matrix as im

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "versalignlib_amd", "csrc", "kernel_instances.hip.h")


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
