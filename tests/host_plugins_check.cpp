// host_plugins_check.cpp -- several kernels of ONE plugin library through the host harness (valign_host.cpp), built with
// -fsanitize=address,undefined together with tests/host_plugins_stub.cpp (tests/test_host_plugins.py, tools/sanitize.sh).
//
// A library has one pair of globals (_parameters / _logger) however many kernels are spawned from it, and vh_spawn points
// them at members of its own vh_plugin.  The rule under test (valign_host.cpp, LibraryGlobals): after vh_close no global
// points into the plugin that was deleted -- a global that held the closing plugin's member moves to the youngest surviving
// plugin of the library, or to null.  The stub's kernel reads the globals in every call, as the reference's kernels do, so
// every call shows whose parameters and whose logger the library holds: before the rule, "score A" after "close B" read
// freed memory.
//
//   open A, open B, score A, score B, close B, score A, open C, close A, score C, close C
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "valign_host.h"

static int failures = 0;

#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            ++failures;                                         \
            fprintf(stderr, "FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            fprintf(stderr, __VA_ARGS__);                       \
            fprintf(stderr, "\n");                              \
        }                                                       \
    } while (0)

static vh_plugin *open_kernel(const char *so, int id, int threads) {
    vh_plugin *p = vh_open(so);
    if (!p) {
        fprintf(stderr, "vh_open: %s\n", vh_last_error());
        exit(2);
    }
    vh_set_param(p, "read_length", id);
    vh_set_param(p, "ref_length", id + 1);
    vh_set_param(p, "num_threads", threads);
    if (vh_spawn(p) != 0) {
        fprintf(stderr, "vh_spawn: %s\n", vh_last_error());
        exit(2);
    }
    return p;
}

// one call of `n` pairs -> the thread count the call saw (the stub writes it into every score)
static int score(vh_plugin *p, int id, int n = 3) {
    std::vector<uint8_t> reads((size_t)n * id, 'A'), refs((size_t)n * (id + 1), 'C');
    std::vector<int16_t> scores((size_t)n, -1);
    const int rc = vh_score(p, 0, n, reads.data(), refs.data(), scores.data());
    CHECK(rc == 0, "vh_score of kernel %d: %s", id, vh_last_error());
    for (int i = 1; i < n; ++i) CHECK(scores[i] == scores[0], "kernel %d: scores differ", id);
    return scores[0];
}

static std::string drain(vh_plugin *p) {
    char buf[4096];
    vh_drain_log(p, buf, sizeof buf);
    return buf;
}

static std::string line(int id, int threads) {
    return "INFO\t[STUB]\tstub " + std::to_string(id) + " score threads=" + std::to_string(threads) + "\n";
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s <stub plugin .so>\n", argv[0]);
        return 2;
    }
    const char *so = argv[1];
    const int A = 11, B = 22, C = 33, tA = 2, tB = 5, tC = 7;
    vh_plugin *a = open_kernel(so, A, tA);
    vh_plugin *b = open_kernel(so, B, tB);          // the library's globals are B's now: both kernels of the stub read them
    int saw = score(a, A);
    CHECK(saw == tB, "score A beside a live B saw %d threads, B's are %d", saw, tB);
    saw = score(b, B);
    CHECK(saw == tB, "score B saw %d threads", saw);
    std::string log = drain(a);
    CHECK(log.empty(), "A's log while the globals are B's: '%s'", log.c_str());
    log = drain(b);
    CHECK(log == line(A, tB) + line(B, tB), "B's log: '%s'", log.c_str());
    vh_close(b);                                    // the globals held B's members: they move to A, the only survivor
    saw = score(a, A);
    CHECK(saw == tA, "score A after close B saw %d threads, the live plugin's are %d", saw, tA);
    log = drain(a);
    CHECK(log == line(A, tA), "A's log after close B: '%s'", log.c_str());
    vh_plugin *c = open_kernel(so, C, tC);          // ... and on to C
    vh_close(a);                                    // A holds neither global: nothing moves
    saw = score(c, C);
    CHECK(saw == tC, "score C after close A saw %d threads", saw);
    log = drain(c);
    CHECK(log == line(C, tC), "C's log: '%s'", log.c_str());
    // vh_reapply_params moves the parameters alone: closing their owner must move them again, the logger stays
    vh_plugin *d = open_kernel(so, A, tA);
    vh_reapply_params(c);
    saw = score(d, A);
    CHECK(saw == tC, "score D after C re-applied its parameters saw %d threads", saw);
    vh_close(c);
    saw = score(d, A);
    CHECK(saw == tA, "score D after close C saw %d threads", saw);
    log = drain(d);
    CHECK(log == line(A, tC) + line(A, tA), "D's log: '%s'", log.c_str());
    vh_close(d);                                    // nobody survives: both globals are null
    vh_plugin *e = vh_open(so);
    CHECK(e != nullptr, "vh_open: %s", vh_last_error());
    if (e) vh_close(e);
    if (failures) return 1;
    printf("host plugins ok\n");
    return 0;
}
