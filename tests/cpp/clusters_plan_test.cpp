// clusters_plan_test.cpp — the host plan of the similar-clusters search (codesearch_amd/csrc/clusters_plan.hpp) on the
// CPU, a stand-alone program: tests/test_similar_clusters_host.py builds it once plain and once under AddressSanitizer +
// UBSan.
//   * the launches cover every tile pair exactly once, in order, none larger than the filter's grid allows; launch 0 is the
//     first tile row; the laboratory knob sets every launch's size;
//   * the ambiguous buffer never holds fewer pairs than one tile pair can produce (128 * 128), whatever the knob;
//   * splitting halves a range into two non-empty parts that tile it, and ends at one tile pair;
//   * the host's walk (ClustersWalk: launch, read the counter, split on overflow, lo half first) accepts every tile pair exactly
//     once and in the triangle's order, with the smallest buffer and the worst load: every tile pair full.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codesearch_amd/csrc/clusters_plan.hpp"
#include "../../include/codesearch_gpu.h"

using namespace cs;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static uint64_t launches_cover(uint64_t rows, uint64_t launch_knob) {
    const ClustersPlan p = plan_clusters(rows, launch_knob, 0);
    CHECK(p.tiles == (rows + 127) / 128);
    CHECK(p.tile_pairs == p.tiles * (p.tiles + 1) / 2);
    CHECK(p.ambiguous_cap == kClustersAmbiguousDefault);
    uint64_t next = 0, launches = 0;
    while (next < p.tile_pairs) {
        const PairsBand b = p.launch_at(next);
        CHECK(b.first == next);
        CHECK(b.count >= 1 && b.count <= kPairsBandTilePairs);
        if (launch_knob) {
            CHECK(b.count == launch_knob || next + b.count == p.tile_pairs);
        } else if (next == 0) {
            CHECK(b.count == p.tiles);  // the first tile row: (0, 0) .. (0, T - 1)
            uint64_t ti = 1, tj = 0;
            tile_pair_of(b.count - 1, p.tiles, ti, tj);
            CHECK(ti == 0 && tj == p.tiles - 1);
        } else {
            CHECK(b.count == p.per_launch || next + b.count == p.tile_pairs);
            CHECK(p.per_launch >= kClustersLaunchMin && (p.per_launch >= p.tile_pairs / 32 || p.per_launch == kPairsBandTilePairs));
            CHECK(launches <= 34 || p.per_launch == kPairsBandTilePairs);
        }
        // the grid of a launch is the pairs filter's: 8 * ceil(count / 8) blocks fit a 32-bit grid
        CHECK(PairsPlan::band_blocks(b.count) >= b.count && PairsPlan::band_blocks(b.count) <= 0xFFFFFFFFull);
        next += b.count;
        ++launches;
    }
    CHECK(next == p.tile_pairs);
    return launches;
}

static void split_ends(uint64_t first, uint64_t count) {
    std::vector<PairsBand> todo{PairsBand{first, count}};
    uint64_t singles = 0, expect = first;
    while (!todo.empty()) {
        const PairsBand r = todo.back();
        todo.pop_back();
        PairsBand lo, hi;
        if (!clusters_split(r, lo, hi)) {
            CHECK(r.count == 1 && r.first == expect);  // lo first: the order of the triangle
            ++expect;
            ++singles;
            continue;
        }
        CHECK(lo.count >= 1 && hi.count >= 1 && lo.count + hi.count == r.count);
        CHECK(lo.first == r.first && hi.first == r.first + lo.count);
        todo.push_back(hi);
        todo.push_back(lo);
    }
    CHECK(singles == count);
}

// The calls' walk (ClustersWalk, as index_joins.hip's clusters_walk drives it) against a device that reports `per_pair`
// ambiguous pairs for every tile pair of a launch.
static void walk(uint64_t rows, uint64_t launch_knob, uint64_t cap_knob, uint64_t per_pair) {
    const ClustersPlan p = plan_clusters(rows, launch_knob, cap_knob);
    CHECK(per_pair <= kClustersTilePairAmbiguous && p.ambiguous_cap >= kClustersTilePairAmbiguous);
    ClustersWalk<ClustersPlan> w(p);
    PairsBand r;
    uint64_t accepted = 0, launches = 0;
    while (w.next(r)) {
        ++launches;
        CHECK(launches <= 4 * p.tile_pairs + 4);  // it ends
        const ClustersStep step = w.report(r, r.count * per_pair);
        CHECK(step != ClustersStep::Impossible);  // a launch that overflowed is never one tile pair
        CHECK((step == ClustersStep::Split) == (r.count * per_pair > p.ambiguous_cap));
        if (step == ClustersStep::Split) continue;
        CHECK(r.first == accepted);  // in order, nothing twice, nothing left out
        accepted += r.count;
    }
    CHECK(accepted == p.tile_pairs);
}

int main() {
    for (uint64_t rows : {0ull, 1ull, 2ull, 127ull, 128ull, 129ull, 1000ull, 100000ull, 1000000ull, 10000000ull})
        for (uint64_t knob : {0ull, 1ull, 2ull, 7ull, 1ull << 20, 1ull << 40}) {
            if (knob && knob < 1000 && rows > 100000) continue;  // (tens of millions of tiny launches: nothing new, minutes)
            launches_cover(rows, knob > kPairsBandTilePairs ? kPairsBandTilePairs : knob);
        }
    CHECK(plan_clusters(0, 0, 0).tile_pairs == 0);
    CHECK(launches_cover(1000, 0) == 2);       // 8 tiles, 36 tile pairs: the first tile row, then the rest
    CHECK(launches_cover(1000, 2) == 18);
    CHECK(plan_clusters(100000, 0, 0).per_launch == 16384 && plan_clusters(100000, 0, 0).first_launch == 782);
    CHECK(plan_clusters(1000000, 0, 0).per_launch == 30525391 / 32 && launches_cover(1000000, 0) == 33);
    CHECK(plan_clusters(10000000, 0, 0).per_launch == kPairsBandTilePairs);
    CHECK(plan_clusters(1000, 1ull << 40, 0).per_launch == kPairsBandTilePairs);  // never past the filter's grid
    // the buffer: never under one tile pair's worth
    CHECK(kClustersTilePairAmbiguous == 16384 && kClustersAmbiguousMin >= kClustersTilePairAmbiguous);
    for (uint64_t knob : {0ull, 1ull, 100ull, 16383ull, 16384ull, 16385ull, 1ull << 20, 1ull << 30})
        CHECK(clusters_ambiguous_cap(knob) >= kClustersAmbiguousMin &&
              (knob < kClustersAmbiguousMin || clusters_ambiguous_cap(knob) == knob));
    CHECK(clusters_ambiguous_cap(0) == kClustersAmbiguousDefault && clusters_ambiguous_cap(1) == 16384);
    CHECK(clusters_ambiguous_cap(1ull << 30) <= 0xFFFFFFFFull && clusters_ambiguous_cap(1ull << 40) == 1ull << 30);
    for (uint64_t count : {1ull, 2ull, 3ull, 36ull, 1000ull, 16384ull, 65537ull}) split_ends(12345, count);
    PairsBand lo, hi;
    CHECK(!clusters_split(PairsBand{5, 1}, lo, hi) && !clusters_split(PairsBand{5, 0}, lo, hi));
    // the walk under the worst load (every tile pair full) and lighter ones, default and knobbed launches
    for (uint64_t rows : {2ull, 129ull, 380ull, 1000ull, 20000ull})
        for (uint64_t launch : {0ull, 1ull, 2ull, 5ull})
            for (uint64_t per_pair : {0ull, 1ull, 8128ull, 16384ull}) {
                walk(rows, launch, 1, per_pair);
                walk(rows, launch, 0, per_pair);
            }
    CHECK(CS_NO_ID == 0xFFFFFFFFu && kClustersNoRoot != kClustersEmptyTile);
    std::printf("clusters plan ok\n");
    return 0;
}
