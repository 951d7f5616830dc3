"""The byte classifier of the kernels' set-up (versalignlib_amd/csrc/base_classes.h) on the CPU: the dword form base_class4
against base_class for all 256 byte values at every byte position.  tests/base_classes_check.cpp includes that header alone
and is built with plain g++ -- no HIP, no GPU."""
import os
import subprocess

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "base_classes_check.cpp")
CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")


def test_base_classes_check(tmp_path):
    exe = str(tmp_path / "base_classes_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert res.returncode == 0 and "base classes ok" in res.stdout, res.stdout[-3000:]


def test_the_kernels_use_the_header_and_hold_no_copy():
    dp = open(os.path.join(CSRC, "dp_kernels.hip.h")).read()
    assert '#include "base_classes.h"' in dp and "int base_class(" not in dp
    assert "base_class4(" in dp
