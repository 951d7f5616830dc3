"""The compact result format on the CPU: vh_cigar_ops / vh_cigar_text of libvalignhost.so (the CPU statement of what the device
encoder of libHIPKernel.so writes) against vh_cigar's strings and a plain-Python restatement (tests/cigar_ref.py), on the
oracle's alignments; the two new entry points and the 24-byte record of include/valign_hip.h."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cigar_ref
from conftest import ROOT
from oracle import cpu_ref
from versalignlib_amd import build, hipkernel, host, synth


def _texts(rows, idx, extended):
    return [host.cigar_text(o) for o in host.cigar_ops(rows, idx, extended=extended)]


def test_known_answer_alignments():
    """The known answers of test_host_and_abi.py::test_cigar_of_known_answer_alignments, both op alphabets, through the ops."""
    reads = host.pad([b"ACGTTTGACC", b"GATTACA", b"AAAA"])
    refs = host.pad([b"ACGTGACC", b"GCATGCT", b"CCCCCCCC"])
    rows, idx = cpu_ref.align(host.NW, reads, refs)
    assert _texts(rows, idx, False) == host.cigars(rows, idx) == ["3M2I5M", "7M", "4M"]
    assert _texts(rows, idx, True) == host.cigars(rows, idx, extended=True) == ["3=2I5=", "1=2X1=1X1=1X", "4X"]
    ops = host.cigar_ops(rows, idx)
    assert [o.tolist() for o in ops] == [[3 << 4 | 0, 2 << 4 | 1, 5 << 4 | 0], [7 << 4], [4 << 4]]
    assert host.cigar_ops(rows, idx, extended=True)[2].tolist() == [4 << 4 | 8]
    rows, idx = cpu_ref.align(host.SW, reads, refs)
    assert _texts(rows, idx, False) == host.cigars(rows, idx) == ["5M", "2M", ""]            # KAT 4: the empty alignment
    assert len(host.cigar_ops(rows, idx)[2]) == 0
    rows, idx = cpu_ref.align(host.NW, host.pad([b"ACGTGACC"]), host.pad([b"ACGTTTGACC"]))
    assert any(int(o) & 15 == 2 for o in host.cigar_ops(rows, idx)[0])                        # a deletion from the read's point of view
    assert host.cigar_text(np.zeros(0, np.uint32)) == ""


@pytest.mark.parametrize("opt", [host.SW, host.NW])
@pytest.mark.parametrize("affine", [False, True])
def test_ops_of_oracle_alignments(opt, affine):
    """A few hundred pairs with indels, lower case and junk bytes: the library's ops are the plain-Python ones, their text is
    vh_cigar's, for both alphabets."""
    reads, refs = synth.make_pairs(300, 60, 90, seed=21 + opt, indel_rate=0.05, n_run_frac=0.1, short_frac=0.2, lowercase_frac=0.1,
                                   junk_frac=0.05)
    sc = cpu_ref.Scoring.make(2, -1, -3, -3, -5, -1, -4, -2) if affine else cpu_ref.Scoring.make()
    rows, idx = cpu_ref.align(opt, reads, refs, sc, threads=4, affine=affine)
    kinds = set()
    for extended in (False, True):
        got = host.cigar_ops(rows, idx, extended=extended)
        exp = cigar_ref.ops_of_rows(rows, idx, extended)
        assert [g.tolist() for g in got] == exp
        assert [host.cigar_text(g) for g in got] == host.cigars(rows, idx, extended=extended)
        kinds |= {o & 15 for e in exp for o in e}
    assert kinds == {0, 1, 2, 7, 8}                     # the case exercises every op


def test_small_cap_is_an_error_not_a_truncation():
    reads = host.pad([b"ACGTTTGACC"])
    refs = host.pad([b"ACGTGACC"])
    rows, idx = cpu_ref.align(host.NW, reads, refs)
    assert len(host.cigar_ops(rows, idx, cap=3)[0]) == 3
    with pytest.raises(host.PluginError, match="too small"):
        host.cigar_ops(rows, idx, cap=2)
    ops = host.cigar_ops(rows, idx)[0]
    buf = ctypes.create_string_buffer(6)                 # "3M2I5M" needs 7 bytes with its NUL
    assert host.lib().vh_cigar_text(ops.ctypes.data, len(ops), buf, len(buf)) == -1
    bad = np.array([5 << 4 | 9], np.uint32)              # no BAM code
    with pytest.raises(host.PluginError):
        host.cigar_text(bad)


def test_longest_run_fits_its_28_bits():
    """R + F < 65536 (the ABI's 16-bit coordinates), so a run is shorter than 2^16: one run of 65534 columns."""
    AL = 65535
    rows = np.zeros((1, 2, AL), np.uint8)
    rows[0, :, :AL - 1] = ord("A")
    idx = np.array([[0, AL - 1, 0, AL - 1]], np.int64)
    ops = host.cigar_ops(rows, idx, extended=True)[0]
    assert ops.tolist() == [(AL - 1) << 4 | 7] and host.cigar_text(ops) == "65534="


def test_entry_points_and_record_size(tmp_path):
    out = subprocess.run(["nm", "-D", "--defined-only", build.HIP_PLUGIN], stdout=subprocess.PIPE, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {"valign_hip_align_cigar_device", "valign_hip_align_cigar_host"} <= names
    assert {"valign_hip_align_cigar_device", "valign_hip_align_cigar_host"} <= set(hipkernel.EXPORTED_SYMBOLS)
    assert hipkernel.aln_dtype().itemsize == 24
    src = os.path.join(ROOT, "tests", "cigar_struct_check.cpp")
    obj = str(tmp_path / "cigar_struct_check.o")
    res = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-c", src, "-o", obj],
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout[-3000:]
