"""The plan of the long-read score path (versalignlib_amd/csrc/long_plan.h: the route of a call, the compiled instances, the
strips' sizes, the banded block chain's plan) on the CPU: tests/long_plan_check.cpp includes the pure header and is built with
plain g++ -- no HIP, no GPU.  The chain's windows, period and kernel variant are compared with the Python statement of the
schedule (tools/band_schedule_model.py), which is itself checked against the oracle (tests/test_band_model.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "long_plan_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
EMPTY = 0x3FFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("long_plan") / "long_plan_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", path],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    return path


def test_long_plan_check(exe):
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "long plan ok" in res.stdout, res.stdout[-3000:]


def test_the_chain_plan_is_the_schedule_model(exe):
    """nb, pad_rows, d, unit_delay and every block's start, lo, span: band_chain_plan against plan(R, F, w, 32, 16)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import band_schedule_model as model
    rng = np.random.default_rng(2025)
    shapes = [(10000, 10000), (10000, 5000)] + [(int(rng.integers(1, 3001)), int(rng.integers(1, 3001))) for _ in range(300)]
    cases = [(R, F, band) for R, F in shapes for band in (2, 16, 64, 512, 100000)]
    res = subprocess.run([exe, "--plans"], input="".join("%d %d %d\n" % c for c in cases), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:]
    lines = res.stdout.split("\n")
    assert len(lines) >= 2 * len(cases)
    units = 0
    for i, (R, F, band) in enumerate(cases):
        head = [int(v) for v in lines[2 * i].split()]
        blocks = [int(v) for v in lines[2 * i + 1].split()]
        pl = model.plan(R, F, band // 2, 32, 16)
        assert head == [R, F, band, pl["nb"], pl["pad"], pl["d"], int(pl["unit"])], (head, pl["d"], pl["unit"])
        exp = []
        for start, lo, hi in zip(pl["start"], pl["lo"], pl["hi"]):
            exp += [start, lo, hi - lo] if lo <= hi else [start, EMPTY, 0]
        assert blocks == exp, (R, F, band)
        units += int(pl["unit"])
    assert 0 < units < len(cases)           # both kernel variants occur


def test_the_engine_has_one_route_and_one_lookup_per_family():
    """The long-read score path decodes its route, sizes its strips, plans the chain and picks its kernels through the checked
    header alone."""
    text = open(os.path.join(CSRC, "engine_long.hip")).read()
    for name in ("long_mode(", "long_strip_sizes(", "long_kernel<", "band_kernel(", "long_instance_exists(", "long_instance_index("):
        assert name in text, name
    for gone in ("kLongNwBand", "nw_kernels[", "single[2][2][2]", "long_geometry<", "make_band_plan"):
        assert gone not in text, gone
    assert "long_single_strip(" not in open(os.path.join(CSRC, "engine_score.hip")).read()
    header = open(os.path.join(CSRC, "long_plan.h")).read()
    for name in ("long_score_mode(", "band_chain_plan(", "hip_runtime"):
        assert (name in header) == (name != "hip_runtime"), name
