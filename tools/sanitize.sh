#!/bin/bash
# CPU-side sanitizer run ("race detection / sanitizers"; the GPU pool offers none):
#   1. the host-only half of the plugin's host-pointer path (versalignlib_amd/csrc/host_pipeline.h: worker pool,
#      gather, scatter) as a stand-alone program under -fsanitize=thread and under -fsanitize=address,undefined;
#      and the engine's cell-range rules and path choice (versalignlib_amd/csrc/cell_rules.h, tests/cell_rules_check.cpp)
#      and the plans of the strip path and of its checkpointed traceback (versalignlib_amd/csrc/strip_plan.h, ckpt_plan.h;
#      tests/strip_plan_check.cpp, tests/ckpt_plan_check.cpp) and of the long-read score path (long_plan.h; tests/long_plan_check.cpp)
#      under -fsanitize=address,undefined;
#   2. libvalignhost.so, valign-bench and the oracle (oracle/cpu_ref.c) built with -fsanitize=address,undefined
#      into build/sanitize/, and the whole CPU test-suite run against THOSE (python gets the runtimes preloaded).
# Usage: tools/sanitize.sh [pytest args...]      (also: make sanitize)
set -eu
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$R/build/sanitize
mkdir -p "$OUT"
CS=$R/versalignlib_amd/csrc
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"

echo "== host_pipeline.h under ThreadSanitizer"
g++ -std=c++17 -O1 -g -fsanitize=thread -fno-omit-frame-pointer -pthread -I"$CS" "$R/tests/host_pipeline_check.cpp" -o "$OUT/host_pipeline_tsan"
TSAN_OPTIONS="halt_on_error=1 second_deadlock_stack=1" "$OUT/host_pipeline_tsan"
echo "== host_pipeline.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -pthread -I"$CS" "$R/tests/host_pipeline_check.cpp" -o "$OUT/host_pipeline_asan"
ASAN_OPTIONS="detect_leaks=1" "$OUT/host_pipeline_asan"
echo "== cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/cell_rules_check.cpp" -o "$OUT/cell_rules_asan"
echo "== ckpt_plan.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/ckpt_plan_check.cpp" -o "$OUT/ckpt_plan_asan"
"$OUT/ckpt_plan_asan"
"$OUT/cell_rules_asan"
echo "== strip_plan.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/strip_plan_check.cpp" -o "$OUT/strip_plan_asan"
"$OUT/strip_plan_asan"
echo "== long_plan.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/long_plan_check.cpp" -o "$OUT/long_plan_asan"
"$OUT/long_plan_asan"
echo "== the band_nw rules of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/band_nw_rules_check.cpp" -o "$OUT/band_nw_rules_asan"
echo "== placed_choice of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/placed_rules_check.cpp" -o "$OUT/placed_rules_asan"
"$OUT/placed_rules_asan"
"$OUT/band_nw_rules_asan"
echo "== placed_choice of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/placed_rules_check.cpp" -o "$OUT/placed_rules_asan"
"$OUT/placed_rules_asan"

echo "== placed_choice under band_placed (cell_rules.h + long_plan.h) under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" -I"$R/include" "$R/tests/placed_band_rules_check.cpp" -o "$OUT/placed_band_rules_asan"
"$OUT/placed_band_rules_asan"

echo "== span_ref_length and span_choice of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/span_rules_check.cpp" -o "$OUT/span_rules_asan"
"$OUT/span_rules_asan"

echo "== subopt_choice of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/subopt_rules_check.cpp" -o "$OUT/subopt_rules_asan"
"$OUT/subopt_rules_asan"

echo "== extend_choice under extend_wide and extend_int32_ok of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_wide_rules_check.cpp" -o "$OUT/extend_wide_rules_asan"
"$OUT/extend_wide_rules_asan"

echo "== extend_choice / extend_align_choice under extend_band, extend_band_int32_ok and the windows of extend_band_plan.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_band_rules_check.cpp" -o "$OUT/extend_band_rules_asan"
"$OUT/extend_band_rules_asan"

echo "== extend_align_choice of cell_rules.h under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_align_rules_check.cpp" -o "$OUT/extend_align_rules_asan"
"$OUT/extend_align_rules_asan"

echo "== the pointer layout of extend_band_align_plan.h and extend_align_choice under extend_band_align under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_band_align_plan_check.cpp" -o "$OUT/extend_band_align_plan_asan"
"$OUT/extend_band_align_plan_asan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_band_align_rules_check.cpp" -o "$OUT/extend_band_align_rules_asan"
"$OUT/extend_band_align_rules_asan"

echo "== extend_zdrop.h (the choices under extend_zdrop, the drop step, the scan's combine, the skip condition) under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_zdrop_rules_check.cpp" -o "$OUT/extend_zdrop_rules_asan"
"$OUT/extend_zdrop_rules_asan"

echo "== extend_zdrop.h (extend_zdrop_rows: the lane form of the drop rule against the serial loop, the choices under the key) under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/extend_zdrop_rows_rules_check.cpp" -o "$OUT/extend_zdrop_rows_rules_asan"
"$OUT/extend_zdrop_rows_rules_asan"

echo "== base_classes.h (the byte classifier of the kernels' set-up) under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/base_classes_check.cpp" -o "$OUT/base_classes_asan"
"$OUT/base_classes_asan"

echo "== lane_map.h (lane <-> group and lane of the group, contiguous and interleaved) under AddressSanitizer + UBSan"
g++ -std=c++17 $SAN -Wall -Werror -I"$CS" "$R/tests/lane_map_check.cpp" -o "$OUT/lane_map_asan"
"$OUT/lane_map_asan"

echo "== several kernels of one plugin library through valign_host.cpp under AddressSanitizer + UBSan"
g++ -std=c++14 $SAN -Wall -Werror -fPIC -shared -I"$R/include" "$R/tests/host_plugins_stub.cpp" -o "$OUT/libStubKernel.so"
g++ -std=c++14 $SAN -Wall -Werror -pthread -I"$R/include" "$R/tests/host_plugins_check.cpp" "$CS/valign_host.cpp" -o "$OUT/host_plugins_asan" -ldl
ASAN_OPTIONS="detect_leaks=1" "$OUT/host_plugins_asan" "$OUT/libStubKernel.so"

echo "== libvalignhost.so, valign-bench, libcpuref.so with $SAN"
g++ -std=c++14 $SAN -fPIC -shared -Wall -pthread -I"$R/include" "$CS/valign_host.cpp" -o "$OUT/libvalignhost.so" -ldl
g++ -std=c++14 $SAN -Wall -I"$R/include" "$CS/valign_bench.cpp" -o "$OUT/valign-bench" -L"$OUT" -lvalignhost -Wl,-rpath,'$ORIGIN' -ldl -pthread
gcc $SAN -fopenmp -fPIC -shared -Wall "$R/oracle/cpu_ref.c" -o "$OUT/libcpuref.so"

echo "== CPU test-suite against the sanitized libraries"
cd "$R"
# python itself is not instrumented: preload the runtimes; leaks are python's own business (detect_leaks=0),
# everything else aborts the test that triggered it
VALIGN_SANITIZED_DIR="$OUT" \
LD_PRELOAD="$(gcc -print-file-name=libasan.so):$(gcc -print-file-name=libubsan.so)" \
ASAN_OPTIONS="detect_leaks=0:abort_on_error=1:allocator_may_return_null=1" \
UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1" \
python -m pytest tests -q -m "not gpu" -p no:cacheprovider "$@"
echo "sanitize: all green"
