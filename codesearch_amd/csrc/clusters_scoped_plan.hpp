// clusters_scoped_plan.hpp — the host side of the scoped similar-clusters search (cs_index_similar_clusters_scoped; kernels:
// scan_clusters_scoped.hip): plain C++17, no HIP.  tests/cpp/clusters_scoped_plan_test.cpp walks it on the CPU;
// index_joins.hip only launches what it says.
//
// GEOMETRY: pairs_scoped_plan.hpp's.  Both sides are packed (list entry i of a scope = packed row i, T = ceil(n / 128)
// packed tiles); the same handle twice is the TRIANGLE of pairs_plan.hpp over T tiles, two handles are the RECTANGLE
// index = ti * TB + tj with the scope of fewer live rows on the A side.  tile_pairs == 0 exactly when the join holds no pair
// whatever the rows are: one list of fewer than two rows, or a side without a row.  (Two handles that hold the same single
// row hold none either; that takes the rows themselves and is the caller's to notice, as there.)
// WALK: clusters_plan.hpp's.  Between two launches the device notes the common root of every packed tile, and a tile pair
// whose two tiles share one is skipped; so the join is walked in launches of `per_launch` tile pairs — a 32nd of them, at
// least kClustersLaunchMin, at most kPairsBandTilePairs — after launch 0, the first tile row (T tile pairs in the triangle,
// TB in the rectangle, capped at per_launch): a file of near-duplicates at the front of a list is one component after it.
// A launch whose ambiguous pairs outgrew the buffer is split by clusters_split, lower half first.  The two laboratory knobs
// are clusters_plan.hpp's, with its clamps.  Every index and product is 64-bit: TA * TB < 2^50 (pairs_scoped_plan.hpp).
#pragma once

#include <cstdint>

#include "clusters_plan.hpp"
#include "pairs_scoped_plan.hpp"

namespace cs {

struct ClustersScopedPlan {
    bool triangle = true;     // same handle: the classes inside one list
    bool swapped = false;     // rectangle: the caller's scope_b is the A side (it holds fewer live rows)
    uint64_t rows_a = 0, rows_b = 0;    // live rows per side, after the swap (triangle: equal)
    uint64_t tiles_a = 0, tiles_b = 0;  // packed tiles per side
    uint64_t tile_pairs = 0;     // 0: no pair whatever the rows hold, nothing is joined
    uint64_t first_launch = 0;   // tile pairs of launch 0
    uint64_t per_launch = 0;     // tile pairs of every later launch (the last may hold fewer)
    uint64_t ambiguous_cap = 0;  // pairs the buffer holds

    // The launch that starts at tile pair `first` (0 <= first < tile_pairs).
    PairsBand launch_at(uint64_t first) const {
        const uint64_t want = first == 0 ? first_launch : per_launch;
        const uint64_t left = tile_pairs - first;
        return PairsBand{first, left < want ? left : want};
    }
    void pair_of(uint64_t index, uint64_t& ti, uint64_t& tj) const {
        if (triangle) tile_pair_of(index, tiles_a, ti, tj);
        else rect_pair_of(index, tiles_b, ti, tj);
    }
};

// live_a / live_b: the lengths of the two lists (same: one list, live_b is not read).  The knobs: plan_clusters'.
inline ClustersScopedPlan plan_clusters_scoped(bool same, uint64_t live_a, uint64_t live_b, uint64_t launch_knob,
                                               uint64_t ambiguous_knob) {
    const PairsScopedPlan g = plan_pairs_scoped(same, live_a, live_b, 1);
    ClustersScopedPlan p;
    p.triangle = g.triangle;
    p.swapped = g.swapped;
    p.rows_a = g.rows_a;
    p.rows_b = g.rows_b;
    p.tiles_a = g.tiles_a;
    p.tiles_b = g.tiles_b;
    p.tile_pairs = g.tile_pairs;
    p.ambiguous_cap = clusters_ambiguous_cap(ambiguous_knob);
    if (launch_knob) {
        p.first_launch = p.per_launch = launch_knob < kPairsBandTilePairs ? launch_knob : kPairsBandTilePairs;
        return p;
    }
    uint64_t per = p.tile_pairs / 32;
    if (per < kClustersLaunchMin) per = kClustersLaunchMin;
    if (per > kPairsBandTilePairs) per = kPairsBandTilePairs;
    p.per_launch = per;
    const uint64_t row = p.tiles_b ? p.tiles_b : 1;  // the first tile row: T (triangle: tiles_b == tiles_a) or TB
    p.first_launch = row < per ? row : per;
    return p;
}

}  // namespace cs
