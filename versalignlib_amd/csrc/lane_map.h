// lane_map.h -- which lane of a wave64 is lane l of lane group grp, one definition for the kernels and a host check.  No HIP here.
//
// A lane group of G lanes owns two pairs; lane l of it owns K consecutive rows and hands its last row to lane l + 1 every
// step (dp_kernels.hip.h).  The hand-over is a DPP move, and a DPP row is 16 lanes: row_shr:n with bound_ctrl writes 0 to the
// lanes whose source would lie before the row's first lane.  Two maps:
//   * CONTIGUOUS (S = 1): group grp is lanes grp * G .. grp * G + G - 1.  l = lane % G, grp = lane / G.  The previous lane of
//     the group is lane - 1.  Groups of 16 ARE the DPP rows, so row_shr:1 with bound_ctrl is "previous lane of my group, 0 in
//     its first lane" in one instruction; a group of 8 or 4 begins in the middle of a row as well, where the shift delivers a
//     neighbour group's value that has to be masked away.
//   * INTERLEAVED (S = 16 / G, G < 16): the S groups of a DPP row sit on alternating lanes -- group (row * S + lane % S), lane
//     l = (lane % 16) / S.  The previous lane of the group is lane - S, in the same row, and the leaders are lanes 0 .. S - 1 of
//     the row: exactly the lanes row_shr:S with bound_ctrl zeroes.  Every group size gets the one-instruction hand-over.
// Either way groups 0 .. 32 / G - 1 are lanes 0 .. 31 (LDS serves a wave's narrow loads a half at a time: the set of groups
// in a half, and so the set of addresses a group-indexed fetch touches per half, is the same under both maps), and the
// butterfly distances of a reduction over the group's lanes are S * G / 2, ..., 2 S, S.
// tests/lane_map_check.cpp checks all of it on the CPU.
#pragma once

#include "cell_constants.h"

#ifndef __HIPCC__       // plain g++ (the CPU check): the functions below are host functions
#define __host__
#define __device__
#endif

#define VALIGN_LANE_MAP_FN __host__ __device__

namespace valign {

constexpr int kLaneMapWave = 64, kDppRowLanes = 16;

template <int G, int S>
struct LaneMap {
    static_assert(G == 4 || G == 8 || G == 16 || G == 32 || G == 64, "group size");
    static_assert(S == 1 || (G < kDppRowLanes && S == kDppRowLanes / G), "the interleaved map puts the 16 / G groups of a DPP row on alternating lanes");
    static constexpr bool kInterleaved = S > 1;
    static constexpr int kGroups = kLaneMapWave / G;
    static constexpr int kStride = S;                      // the previous lane of my group is lane - S
    // the DPP control of the hand-over: row_shr:S.  With bound_ctrl it is 0 in the leaders where the map is interleaved or
    // G == 16; a contiguous group of 8 or 4 has leaders inside a row (is_leader), which the shift does not zero
    static constexpr int kRowShr = 0x110 + S;
    static constexpr bool kRowShrZeroesLeaders = kInterleaved || G == kDppRowLanes;
    // butterfly distances of a reduction over the G lanes of a group, largest first
    static constexpr int kReduceSteps = G == 4 ? 2 : G == 8 ? 3 : G == 16 ? 4 : G == 32 ? 5 : 6;
    VALIGN_LANE_MAP_FN static constexpr int reduce_distance(int i) { return S * (G / 2 >> i); }

    VALIGN_LANE_MAP_FN static constexpr int l(int lane) { return kInterleaved ? (lane % kDppRowLanes) / S : lane % G; }
    VALIGN_LANE_MAP_FN static constexpr int grp(int lane) { return kInterleaved ? (lane / kDppRowLanes) * S + lane % S : lane / G; }
    VALIGN_LANE_MAP_FN static constexpr int lane_of(int grp, int l) {
        return kInterleaved ? (grp / S) * kDppRowLanes + l * S + grp % S : grp * G + l;
    }
    VALIGN_LANE_MAP_FN static constexpr bool is_leader(int lane) { return l(lane) == 0; }
    // (of a lane that is no leader)
    VALIGN_LANE_MAP_FN static constexpr int prev_lane(int lane) { return lane - S; }
};

// The lane stride of a geometry's score kernel.  Interleaved for the 8 x 19 side tile alone: every other kernel of 8- or 4-lane
// groups fetches an LDS profile whose slab stride profile_conflicts() (dp_kernels.hip.h) chose for the contiguous map.
constexpr int score_lane_stride(int G, int K) { return tilt_tables_only(G, K) ? kDppRowLanes / G : 1; }

}  // namespace valign
