// lane_map_check.cpp -- CPU check of versalignlib_amd/csrc/lane_map.h (plain g++, no HIP; tests/test_lane_map.py builds and runs
// it, tools/sanitize.sh runs it under AddressSanitizer + UBSan).  For the contiguous map of 8- and 16-lane groups and the
// interleaved one of 8- and 4-lane groups: lane <-> (group, lane of the group) is a bijection; the previous lane of a group is
// S lanes back in the same 16-lane DPP row; the lanes whose row_shr:S source lies outside the row are exactly the leaders where
// the map says the shift zeroes them; the butterfly distances of a group reduction reach the G lanes of the group and no other;
// and groups 0 .. 3 are lanes 0 .. 31 under both maps of 8-lane groups.
#include <stdio.h>

#include <initializer_list>
#include <set>

#include "lane_map.h"

using namespace valign;

static int failures = 0;

#define CHECK(...)                                                           \
    do {                                                                     \
        if (!(__VA_ARGS__)) {                                                \
            if (++failures < 20) printf("FAILED line %d: %s\n", __LINE__, #__VA_ARGS__); \
        }                                                                    \
    } while (0)

template <int G, int S>
static void check_map() {
    using map = LaneMap<G, S>;
    CHECK(map::kGroups * G == kLaneMapWave && map::kStride == S && map::kRowShr == 0x110 + S && map::kInterleaved == (S > 1));
    // a bijection, both ways
    std::set<int> seen;
    for (int lane = 0; lane < kLaneMapWave; ++lane) {
        const int g = map::grp(lane), l = map::l(lane);
        CHECK(g >= 0 && g < map::kGroups && l >= 0 && l < G);
        CHECK(map::lane_of(g, l) == lane);
        seen.insert(g * G + l);
    }
    CHECK((int)seen.size() == kLaneMapWave);
    for (int g = 0; g < map::kGroups; ++g)
        for (int l = 0; l < G; ++l) {
            const int lane = map::lane_of(g, l);
            CHECK(lane >= 0 && lane < kLaneMapWave && map::grp(lane) == g && map::l(lane) == l);
        }
    // the previous lane of the group: S lanes back, in the same DPP row
    for (int lane = 0; lane < kLaneMapWave; ++lane) {
        CHECK(map::is_leader(lane) == (map::l(lane) == 0));
        if (map::is_leader(lane)) continue;
        const int prev = map::prev_lane(lane);
        CHECK(prev == lane - S && map::grp(prev) == map::grp(lane) && map::l(prev) == map::l(lane) - 1);
        if (G <= kDppRowLanes) CHECK(prev / kDppRowLanes == lane / kDppRowLanes);
    }
    // row_shr:S with bound_ctrl writes 0 where lane % 16 < S: exactly the leaders, where the map promises it
    int zeroed_leaders = 0, leaders = 0;
    for (int lane = 0; lane < kLaneMapWave; ++lane) {
        const bool zeroed = lane % kDppRowLanes < S;
        leaders += map::is_leader(lane);
        zeroed_leaders += zeroed && map::is_leader(lane);
        if (map::kRowShrZeroesLeaders) CHECK(zeroed == map::is_leader(lane));
        else CHECK(!zeroed || map::is_leader(lane));               // (a contiguous group of 8: the shift zeroes every other leader only)
    }
    CHECK(leaders == map::kGroups);
    CHECK(map::kRowShrZeroesLeaders == (zeroed_leaders == leaders));
    // the butterfly: from any lane the distances reach the G lanes of its group, each once, and nothing else
    int steps = 0;
    for (int g = G; g > 1; g >>= 1) ++steps;
    CHECK(map::kReduceSteps == steps);
    for (int i = 0; i + 1 < map::kReduceSteps; ++i) CHECK(map::reduce_distance(i) == 2 * map::reduce_distance(i + 1));
    CHECK(map::reduce_distance(map::kReduceSteps - 1) == S && map::reduce_distance(0) == S * G / 2);
    for (int lane = 0; lane < kLaneMapWave; ++lane) {
        std::set<int> reached;
        for (int mask = 0; mask < (1 << map::kReduceSteps); ++mask) {
            int at = lane;
            for (int i = 0; i < map::kReduceSteps; ++i)
                if (mask >> i & 1) at ^= map::reduce_distance(i);
            CHECK(at >= 0 && at < kLaneMapWave && map::grp(at) == map::grp(lane));
            reached.insert(at);
        }
        CHECK((int)reached.size() == G);
    }
    // the first half of the wave holds the first half of the groups (LDS serves narrow loads 32 lanes at a time)
    for (int lane = 0; lane < kLaneMapWave; ++lane) CHECK((lane < 32) == (map::grp(lane) < map::kGroups / 2));
}

int main() {
    check_map<8, 1>();
    check_map<8, 2>();
    check_map<4, 4>();
    check_map<16, 1>();
    // both maps of 8-lane groups put groups 0 .. 3 into lanes 0 .. 31; the interleaved one puts group 2r on the even lanes of DPP
    // row r and group 2r + 1 on the odd ones
    for (int lane = 0; lane < kLaneMapWave; ++lane) {
        CHECK((LaneMap<8, 1>::grp(lane) < 4) == (lane < 32) && (LaneMap<8, 2>::grp(lane) < 4) == (lane < 32));
        CHECK(LaneMap<8, 2>::grp(lane) == 2 * (lane / 16) + lane % 2 && LaneMap<8, 2>::l(lane) == (lane % 16) / 2);
        CHECK(LaneMap<8, 1>::grp(lane) == lane / 8 && LaneMap<8, 1>::l(lane) == lane % 8);
        CHECK(LaneMap<4, 4>::grp(lane) == 4 * (lane / 16) + lane % 4 && LaneMap<4, 4>::l(lane) == (lane % 16) / 4);
    }
    // the trait: interleaved for the 8 x 19 side tile and nothing else
    static_assert(score_lane_stride(kSideTileG, kSideTileK) == 2, "the side tile interleaves its two groups per DPP row");
    for (int G : {4, 8, 16, 32, 64})
        for (int K = 2; K <= 32; ++K) CHECK(score_lane_stride(G, K) == (G == 8 && K == 19 ? 2 : 1));
    CHECK(LaneMap<8, 2>::kRowShrZeroesLeaders && LaneMap<4, 4>::kRowShrZeroesLeaders && LaneMap<16, 1>::kRowShrZeroesLeaders && !LaneMap<8, 1>::kRowShrZeroesLeaders);
    CHECK(LaneMap<8, 2>::reduce_distance(0) == 8 && LaneMap<8, 2>::reduce_distance(1) == 4 && LaneMap<8, 2>::reduce_distance(2) == 2);

    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("lane map ok\n");
    return 0;
}
