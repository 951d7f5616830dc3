// host_plugins_stub.cpp -- a versalignLib plugin without a kernel, for tests/host_plugins_check.cpp: the four exported symbols
// and the two globals, used the way the reference's kernels use the protocol -- the kernel object keeps nothing of the host's:
// num_threads is read from the global parameter object in every call (DefaultKernel.cpp:45) and every line goes to the global
// logger (the `Parameters` / `Logger` macros).  So whatever the host leaves in the globals is what a call touches.
#include <stdio.h>

#include "versalign_plugin_abi.h"

#define STUB_EXPORT __attribute__((visibility("default")))

STUB_EXPORT AlignmentParameters *_parameters = 0;
STUB_EXPORT AlignmentLogger *_logger = 0;

namespace {

class StubKernel : public AlignmentKernel {
public:
    StubKernel() {
        if (!_parameters || !Parameters.has_key("read_length")) throw "Cannot instantiate Kernel. Lacking parameters";
        id_ = Parameters.param_int("read_length");          // (the check gives every kernel a read_length of its own)
    }
    // one line per call; every score is the thread count the call saw
    void score_alignments(int const &, int const &aln_number, char const *const *const, char const *const *const,
                          short *const scores) override {
        const int threads = Parameters.param_int("num_threads");
        char line[96];
        snprintf(line, sizeof line, "stub %d score threads=%d", id_, threads);
        Logger.log(0, "STUB", line);
        for (int i = 0; i < aln_number; ++i) scores[i] = (short)threads;
    }
    void compute_alignments(int const &, int const &, char const *const *const, char const *const *const, Alignment *const) override {}

private:
    int id_ = 0;
};

}  // namespace

extern "C" {
STUB_EXPORT AlignmentKernel *spawn_alignment_kernel() { return new StubKernel(); }
STUB_EXPORT void set_parameters(AlignmentParameters *parameters) { _parameters = parameters; }
STUB_EXPORT void set_logger(AlignmentLogger *logger) { _logger = logger; }
STUB_EXPORT void delete_alignment_kernel(AlignmentKernel *instance) { delete instance; }
}
