// align_parts.h -- the register path of an alignment call (Engine::align_device) before its launches: how much of the batch
// the pointer scratch takes at a time, and the parts the batch is cut into.  Integers in, integers out; no HIP.
#pragma once

#include <stddef.h>

#include <algorithm>
#include <vector>

namespace valign {

struct TraceScratch {
    int blocks8 = 0;                // blocks of steps per lane
    size_t bytes_per_pp = 0;        // pointer-stream bytes of a pair-of-pairs
    long long ppb = 0;              // pairs per block
    long long chunk = 0;            // pairs the scratch is sized for
    long long chain_pairs = 0;      // pairs of one region of a chained call
    bool chained = false;           // the call keeps its chain (two regions fit)
};

// Pointer scratch: as much of the batch per launch as memory allows (a 1 M-pair launch keeps
// the traceback kernel at full occupancy), capped at 64 GiB -- one launch for a million affine pairs of
// 150 x 500 (43.6 GB) on a 288 GB device -- and half the free HBM (`free_b`: free bytes plus the scratch held already).
// chain_chunk_pairs: the chunk size of a chained call (WalkChain), 0 = not chained
inline TraceScratch size_trace_scratch(int G, int K, int F, bool affine, bool affine_tagged, long long ppb, size_t free_b,
                                       long long scratch_cap_mb, long long n, long long chain_chunk_pairs, bool no_overlap) {
    TraceScratch s;
    s.blocks8 = affine_tagged ? (F + G - 1 + 3) / 4 : (F + G - 1 + 7) / 8;
    s.ppb = ppb;
    s.bytes_per_pp = (size_t)G * s.blocks8 * K * 4 * ((affine && !affine_tagged) ? 2 : 1);
    size_t cap = std::min<size_t>(64ull << 30, std::max<size_t>(free_b / 2, 256ull << 20));
    if (scratch_cap_mb > 0) cap = std::min<size_t>(cap, (size_t)scratch_cap_mb << 20);
    long long chunk = (long long)(cap / s.bytes_per_pp) * 2;
    chunk = std::max(ppb, chunk / ppb * ppb);
    s.chain_pairs = chain_chunk_pairs > 0 ? (std::max(chain_chunk_pairs, n) + ppb - 1) / ppb * ppb : 0;
    s.chained = chain_chunk_pairs > 0 && !(2 * s.chain_pairs > chunk || no_overlap);        // two regions do not fit: stream order
    s.chunk = s.chained ? 2 * s.chain_pairs : std::min(chunk, (n + ppb - 1) / ppb * ppb);
    return s;
}

struct Part {
    long long begin, cnt, slot;     // pairs [begin, begin + cnt) of the batch, from pair `slot` of the scratch on
    int region;                     // 0 / 1: whose fill_done / trace_done events the part uses
};

// Parts of the batch: the traceback of one part runs on a helper stream beside the fill of the next (the walk
// waits on memory at 17 % VALU issue, the fill owns the VALU).  A batch that fits the scratch in one piece is cut
// 7/8 + 1/8 -- the short fill covers the long walk, what stays exposed is the walk of the last eighth (cuts between
// 3/4 and 7/8 measure the same, finer ones lose to the second fill's own tail); a batch
// that needs several chunks alternates between the two halves of the scratch.
// chain_region: region of a chained call (the whole batch is one part there), -1 = not chained;
// overlap: walks may run beside fills (a batch of 1e10 cells or more, switch no_overlap off)
inline std::vector<Part> cut_parts(long long n, const TraceScratch &s, int chain_region, bool overlap) {
    std::vector<Part> parts;
    const long long ppb = s.ppb, chunk = s.chunk;
    if (chain_region >= 0) {
        parts.push_back(Part{0, n, chain_region * s.chain_pairs, chain_region});
    } else if (overlap && chunk >= n && n >= 16 * ppb) {
        const long long big = std::max(ppb, n * 7 / 8 / ppb * ppb);
        parts.push_back(Part{0, big, 0, 0});
        parts.push_back(Part{big, n - big, big, 1});
    } else if (overlap && chunk < n && chunk >= 4 * ppb) {
        const long long half = chunk / 2 / ppb * ppb;
        for (long long begin = 0, i = 0; begin < n; begin += half, ++i)
            parts.push_back(Part{begin, std::min(half, n - begin), (i & 1) * half, (int)(i & 1)});
    } else {
        for (long long begin = 0; begin < n; begin += chunk) parts.push_back(Part{begin, std::min(chunk, n - begin), 0, 0});
    }
    return parts;
}

}  // namespace valign
