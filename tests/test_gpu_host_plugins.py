"""Two live kernels of libHIPKernel.so through the host harness: each keeps, for its whole life, the parameters and the logger
it was spawned with (tests/test_host_plugins.py runs the harness's side of it on the CPU under sanitizers)."""
import numpy as np
import pytest

from oracle import cpu_ref
from versalignlib_amd import build, host, synth

pytestmark = pytest.mark.gpu


def test_two_live_kernels_keep_their_own_parameters_and_log():
    R, F, n = 64, 128, 200
    reads, refs = synth.make_pairs(n, R, F, seed=21, indel_rate=0.02, n_run_frac=0.05, short_frac=0.1)
    a = b = None
    try:
        a = host.Plugin(build.HIP_PLUGIN, R, F, num_threads=1)
        b = host.Plugin(build.HIP_PLUGIN, R, F, num_threads=4, ragged_batching=1)
        a.drain_log()
        b.drain_log()
        got = a.score_alignments(host.SW, reads, refs)
        log_a, log_b = a.drain_log(), b.drain_log()
        assert "with 1 host threads" in log_a and '"ragged_batching": 0' in log_a, log_a
        assert "with 4 host threads" not in log_a and '"ragged_batching": 1' not in log_a, log_a
        assert log_b == "", log_b
        assert np.array_equal(got, cpu_ref.score(host.SW, reads, refs, threads=4))
        b.score_alignments(host.SW, reads[:8], refs[:8])
        log_a, log_b = a.drain_log(), b.drain_log()
        assert log_a == "" and "with 4 host threads" in log_b and '"ragged_batching": 1' in log_b, (log_a, log_b)
        b.close()
        for opt in (host.SW, host.NW):
            assert np.array_equal(a.score_alignments(opt, reads, refs), cpu_ref.score(opt, reads, refs, threads=4)), opt
            rows, idx = a.compute_alignments(opt, reads, refs)
            erows, eidx = cpu_ref.align(opt, reads, refs, threads=4)
            assert np.array_equal(idx, eidx) and np.array_equal(rows, erows), opt
        assert "with 1 host threads" in a.drain_log()
    finally:
        for plug in (b, a):
            if plug is not None:
                plug.close()
