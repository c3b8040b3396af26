// clusters_plan.hpp — the host side of the similar-clusters search (cs_index_similar_clusters; kernels: scan_clusters.hip):
// plain C++17, no HIP.  tests/cpp/clusters_plan_test.cpp walks it on the CPU; index_joins.hip only launches what it says.
//
// The join is the similar-pairs search's: the upper triangle of T x T 128-row tiles in pairs_plan.hpp's numbering (row by
// row, the diagonal pair first; tile_pair_of).  What differs is the walk.  The answer is a union-find over the stored rows,
// and between two launches the device notes, per tile, the common root of its live rows (tile_root): a tile pair whose two
// tiles share one root can add nothing and is skipped after one comparison.  A launch only profits from the unions of the
// launches before it, so the triangle is walked in more launches than the pairs call's bands:
//   launch 0     the first tile row (T tile pairs): a contiguous file of near-duplicates at the front of the store is one
//                component after it, and the rest of its triangle is skipped;
//   launch k > 0 `per_launch` consecutive tile pairs: a 32nd of the triangle, at least 16,384, at most kPairsBandTilePairs
//                (the filter's grid).  Skipping only matters for a file that is a large share of the store — rows that are
//                a fifth of it are 4 % of the tile pairs — and such a file spans several 32nds.  Shorter launches are not
//                free: every launch ends in a drain and a host synchronise, and at 1M rows 246 launches instead of 30
//                cost 8 % (977: 11 %; measured).
// Pairs the f16 product cannot decide (within the margin of the bound: "ambiguous") go to ONE buffer of fixed size, consumed
// and reused after every launch.  A launch that counted more of them than the buffer holds is SPLIT in two halves which are
// scored again (uniting is idempotent); a launch of one tile pair holds at most 128 * 128 = 16,384, and the buffer never
// holds fewer, so splitting ends.
#pragma once

#include <cstdint>
#include <vector>

#include "pairs_plan.hpp"

namespace cs {

constexpr uint64_t kClustersTilePairAmbiguous = (uint64_t)kPairsTileRows * kPairsTileRows;  // 16,384
constexpr uint64_t kClustersAmbiguousMin = kClustersTilePairAmbiguous;
constexpr uint64_t kClustersAmbiguousDefault = 1ull << 20;  // 8 MiB of (rowA | rowB << 32)
constexpr uint64_t kClustersLaunchMin = 16384;
constexpr uint32_t kClustersNoRoot = 0xFFFFFFFFu;     // tile_root: the tile's live rows have no common root
constexpr uint32_t kClustersEmptyTile = 0xFFFFFFFEu;  // tile_root: the tile has no live row

// The ambiguous buffer's capacity: `knob` (a laboratory setting; 0 = none) or the default, never under the minimum.
inline uint64_t clusters_ambiguous_cap(uint64_t knob) {
    const uint64_t want = knob ? knob : kClustersAmbiguousDefault;
    if (want > (1ull << 30)) return 1ull << 30;  // the kernels count the buffer's slots in 32 bits
    return want < kClustersAmbiguousMin ? kClustersAmbiguousMin : want;
}

struct ClustersPlan {
    uint64_t tiles = 0;          // T
    uint64_t tile_pairs = 0;     // T (T + 1) / 2
    uint64_t first_launch = 0;   // tile pairs of launch 0
    uint64_t per_launch = 0;     // tile pairs of every later launch (the last may hold fewer)
    uint64_t ambiguous_cap = 0;  // pairs the buffer holds

    // The launch that starts at tile pair `first` (0 <= first < tile_pairs).
    PairsBand launch_at(uint64_t first) const {
        const uint64_t want = first == 0 ? first_launch : per_launch;
        const uint64_t left = tile_pairs - first;
        return PairsBand{first, left < want ? left : want};
    }
};

// `launch_knob` (a laboratory setting; 0 = none): every launch, the first included, holds that many tile pairs.
inline ClustersPlan plan_clusters(uint64_t stored_rows, uint64_t launch_knob, uint64_t ambiguous_knob) {
    ClustersPlan p;
    p.tiles = (stored_rows + kPairsTileRows - 1) / kPairsTileRows;
    p.tile_pairs = tile_pairs_of(p.tiles);
    p.ambiguous_cap = clusters_ambiguous_cap(ambiguous_knob);
    if (launch_knob) {
        p.first_launch = p.per_launch = launch_knob < kPairsBandTilePairs ? launch_knob : kPairsBandTilePairs;
        return p;
    }
    uint64_t per = p.tile_pairs / 32;
    if (per < kClustersLaunchMin) per = kClustersLaunchMin;
    if (per > kPairsBandTilePairs) per = kPairsBandTilePairs;
    p.per_launch = per;
    p.first_launch = p.tiles < per ? (p.tiles ? p.tiles : 1) : per;
    return p;
}

// A launch whose ambiguous pairs did not fit: its two halves, lo first.  false: it holds one tile pair and cannot be
// split — which never happens to a launch that overflowed, since one tile pair fits the smallest buffer.
inline bool clusters_split(const PairsBand& r, PairsBand& lo, PairsBand& hi) {
    if (r.count < 2) return false;
    lo = PairsBand{r.first, r.count / 2};
    hi = PairsBand{r.first + lo.count, r.count - lo.count};
    return true;
}

// What a launch's ambiguous count means to the walk.
enum class ClustersStep {
    Accepted,   // within the buffer: the launch stands, its ambiguous pairs go to the rescore
    Split,      // past it: the launch is void, its two halves are walked instead
    Impossible  // past it in a launch of one tile pair, which holds at most kClustersTilePairAmbiguous: the count is wrong
};

// The walk of both clusters calls over `plan` (ClustersPlan, ClustersScopedPlan: tile_pairs, launch_at, ambiguous_cap) —
// what to launch next, and what becomes of a launch once its ambiguous pairs are counted.  It touches no device:
// index_joins.hip's clusters_walk launches what next() says and reports the counter it read; the plans' tests report a
// made-up one.  The plan outlives the walk.
template <typename Plan>
class ClustersWalk {
public:
    explicit ClustersWalk(const Plan& plan) : plan_(plan) {}

    // r = the next launch: a half that is waiting (lo before hi, so the walk stays in the plan's order), else the plan's
    // next launch.  false: every tile pair has been accepted, the walk has ended.
    bool next(PairsBand& r) {
        if (!halves_.empty()) {
            r = halves_.back();
            halves_.pop_back();
            return true;
        }
        if (next_ >= plan_.tile_pairs) return false;
        r = plan_.launch_at(next_);
        next_ += r.count;
        return true;
    }

    // The launch `r` that next() gave counted `ambiguous` pairs.
    ClustersStep report(const PairsBand& r, uint64_t ambiguous) {
        if (ambiguous <= plan_.ambiguous_cap) return ClustersStep::Accepted;
        PairsBand lo, hi;
        if (!clusters_split(r, lo, hi)) return ClustersStep::Impossible;
        halves_.push_back(hi);
        halves_.push_back(lo);
        return ClustersStep::Split;
    }

private:
    const Plan& plan_;
    std::vector<PairsBand> halves_;  // of launches whose ambiguous pairs did not fit; the next to walk is at the back
    uint64_t next_ = 0;              // the first tile pair no launch has named yet
};

}  // namespace cs
