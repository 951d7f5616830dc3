"""Several kernels of one plugin library through the host harness, on the CPU under AddressSanitizer + UBSan:
tests/host_plugins_check.cpp drives versalignlib_amd/csrc/valign_host.cpp against tests/host_plugins_stub.cpp, a plugin whose
kernel reads the library's globals in every call.  The program carries its own runtime; nothing is preloaded."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "versalignlib_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def _gxx(args):
    build = subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-pthread", "-I" + INCLUDE] + SAN + args,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout[-3000:]


def test_kernels_of_one_library_under_sanitizers(tmp_path):
    stub, exe = str(tmp_path / "libStubKernel.so"), str(tmp_path / "host_plugins_asan")
    _gxx(["-fPIC", "-shared", os.path.join(ROOT, "tests", "host_plugins_stub.cpp"), "-o", stub])
    _gxx([os.path.join(ROOT, "tests", "host_plugins_check.cpp"), os.path.join(CSRC, "valign_host.cpp"), "-o", exe, "-ldl"])
    # The child runs without LD_PRELOAD, as tests/test_sanitizers.py runs its program: it is linked against the ASan / UBSan
    # runtime itself, and ASan refuses to start when any preloaded library comes before its runtime (`make sanitize` preloads
    # the runtimes for python).  Dropping a preload is harmless here: the child is a CPU-only program -- the harness and a
    # stub plugin, no HIP, no GPU library -- so a preload meant for processes that use the GPU has nothing to act on in it.
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    env["ASAN_OPTIONS"] = "detect_leaks=1"
    res = subprocess.run([exe, stub], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, env=env)
    assert res.returncode == 0 and "host plugins ok" in res.stdout, res.stdout[-3000:]
    assert "ERROR: AddressSanitizer" not in res.stdout and "runtime error" not in res.stdout, res.stdout[-3000:]

