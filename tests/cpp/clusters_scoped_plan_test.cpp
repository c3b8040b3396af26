// clusters_scoped_plan_test.cpp — the host plan of the scoped similar-clusters search
// (codesearch_amd/csrc/clusters_scoped_plan.hpp) on the CPU, a stand-alone program: tests/test_similar_clusters_scoped_host.py
// builds it once plain and once under AddressSanitizer + UBSan.
//   * the launches cover triangle and rectangle exactly once, in order — every tile pair named, exhaustively, for T, TA, TB
//     in 1 .. 40 — and at 78,125 x 78,125 tiles with the launches' ends sampled; launch 0 is the first tile row;
//   * the two laboratory knobs and their clamps;
//   * halves tile their parent and splitting ends at one tile pair; the host's walk (clusters_plan.hpp ClustersWalk) under the
//     worst load accepts every tile pair once, in order;
//   * the three empty joins: a side without a row, one list of fewer than two rows (the same single row behind two handles is
//     the caller's to notice: the plan says one tile pair).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codesearch_amd/csrc/clusters_scoped_plan.hpp"
#include "../../include/codesearch_gpu.h"

using namespace cs;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

// Rows that make exactly `tiles` packed tiles with a ragged last one.
static uint64_t rows_of(uint64_t tiles) { return tiles * 128 - 5; }

// Walks the plan's launches; exhaustive: names every tile pair of every launch and checks it against the numbering.
static uint64_t launches_cover(const ClustersScopedPlan& p, uint64_t launch_knob, bool exhaustive) {
    const uint64_t row0 = p.tiles_b;  // the first tile row: T (triangle: tiles_b == tiles_a) or TB
    uint64_t next = 0, launches = 0, ei = 0, ej = 0;  // (ei, ej): the tile pair expected next
    while (next < p.tile_pairs) {
        const PairsBand b = p.launch_at(next);
        CHECK(b.first == next);
        CHECK(b.count >= 1 && b.count <= kPairsBandTilePairs);
        if (launch_knob) {
            CHECK(b.count == launch_knob || next + b.count == p.tile_pairs);
        } else if (next == 0) {
            CHECK(b.count == (row0 < p.per_launch ? row0 : p.per_launch));
            uint64_t ti = 1, tj = 0;
            p.pair_of(b.count - 1, ti, tj);
            CHECK(ti == 0 && tj == b.count - 1);  // (0, 0) .. : launch 0 stays in tile row 0
        } else {
            CHECK(b.count == p.per_launch || next + b.count == p.tile_pairs);
            CHECK(p.per_launch >= kClustersLaunchMin && (p.per_launch >= p.tile_pairs / 32 || p.per_launch == kPairsBandTilePairs));
            CHECK(launches <= 34 || p.per_launch == kPairsBandTilePairs);
        }
        CHECK(PairsPlan::band_blocks(b.count) >= b.count && PairsPlan::band_blocks(b.count) <= 0xFFFFFFFFull);
        for (uint64_t idx : {b.first, b.first + b.count - 1}) {  // a launch's ends land inside the join
            uint64_t ti = ~0ull, tj = ~0ull;
            p.pair_of(idx, ti, tj);
            CHECK(ti < p.tiles_a && tj < p.tiles_b);
            if (p.triangle) CHECK(ti <= tj);
            else CHECK(rect_index_of(ti, tj, p.tiles_b) == idx);
        }
        if (exhaustive)
            for (uint64_t idx = b.first; idx < b.first + b.count; ++idx) {
                uint64_t ti = ~0ull, tj = ~0ull;
                p.pair_of(idx, ti, tj);
                CHECK(ti == ei && tj == ej);
                if (++ej == p.tiles_b) { ++ei; ej = p.triangle ? ei : 0; }
            }
        next += b.count;
        ++launches;
    }
    CHECK(next == p.tile_pairs);
    if (exhaustive && p.tile_pairs) CHECK(ei == p.tiles_a);
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
            CHECK(r.count == 1 && r.first == expect);  // lo first: the order of the join
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
static void walk(const ClustersScopedPlan& p, uint64_t per_pair) {
    CHECK(per_pair <= kClustersTilePairAmbiguous && p.ambiguous_cap >= kClustersTilePairAmbiguous);
    ClustersWalk<ClustersScopedPlan> w(p);
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
    // geometry: pairs_scoped_plan.hpp's, whatever the knobs
    for (uint64_t knob : {0ull, 1ull, 2ull, 7ull}) {
        for (uint64_t T = 1; T <= 40; ++T) {
            const ClustersScopedPlan t = plan_clusters_scoped(true, rows_of(T), 999, knob, 0);
            CHECK(t.triangle && !t.swapped && t.rows_a == rows_of(T) && t.rows_b == t.rows_a && t.tiles_a == T && t.tiles_b == T);
            CHECK(t.tile_pairs == tile_pairs_of(T) && t.ambiguous_cap == kClustersAmbiguousDefault);
            launches_cover(t, knob, true);
            for (uint64_t TB = 1; TB <= 40; ++TB) {
                const ClustersScopedPlan r = plan_clusters_scoped(false, rows_of(T), rows_of(TB), knob, 0);
                CHECK(!r.triangle && r.swapped == (TB < T));  // the smaller side on A
                CHECK(r.tiles_a == (T < TB ? T : TB) && r.tiles_b == (T < TB ? TB : T) && r.tile_pairs == T * TB);
                CHECK(r.rows_a == rows_of(r.tiles_a) && r.rows_b == rows_of(r.tiles_b));
                launches_cover(r, knob, true);
            }
        }
    }
    // launch 0 is the first tile row; small joins are two launches
    CHECK(plan_clusters_scoped(true, 1000, 0, 0, 0).first_launch == 8 && launches_cover(plan_clusters_scoped(true, 1000, 0, 0, 0), 0, true) == 2);
    CHECK(plan_clusters_scoped(false, 300, 1000, 0, 0).first_launch == 8 && plan_clusters_scoped(false, 1000, 300, 0, 0).first_launch == 8);
    CHECK(launches_cover(plan_clusters_scoped(false, 300, 1000, 0, 0), 0, true) == 2);  // 3 x 8: one row of 8, then 16
    CHECK(launches_cover(plan_clusters_scoped(true, 1000, 0, 2, 0), 2, true) == 18);
    CHECK(launches_cover(plan_clusters_scoped(true, 2, 0, 0, 0), 0, true) == 1);
    // the triangle of a scope walks as the unscoped plan does for as many stored rows
    for (uint64_t n : {2ull, 129ull, 1000ull, 100000ull, 1000000ull, 10000000ull}) {
        const ClustersScopedPlan s = plan_clusters_scoped(true, n, 0, 0, 0);
        const ClustersPlan u = plan_clusters(n, 0, 0);
        CHECK(s.tile_pairs == u.tile_pairs && s.first_launch == u.first_launch && s.per_launch == u.per_launch);
        launches_cover(s, 0, false);
    }
    CHECK(plan_clusters_scoped(true, 1000000, 0, 0, 0).per_launch == 30525391 / 32);
    CHECK(launches_cover(plan_clusters_scoped(true, 1000000, 0, 0, 0), 0, false) == 33);
    // a 10 % scope against its complement at 1M rows: 782 x 7,032 tile pairs, about 18 % of the store's triangle
    const ClustersScopedPlan rc = plan_clusters_scoped(false, 900000, 100000, 0, 0);
    CHECK(rc.swapped && rc.tiles_a == 782 && rc.tiles_b == 7032 && rc.tile_pairs == 782ull * 7032ull && rc.first_launch == 7032);
    CHECK(rc.per_launch == rc.tile_pairs / 32 && launches_cover(rc, 0, false) == 33);
    CHECK(rc.tile_pairs * 100 / tile_pairs_of(7813) == 18);
    // 78,125 x 78,125 tiles (all of 10M rows on both sides; 6.1e9 tile pairs): 64-bit throughout, the launches' ends sampled
    const ClustersScopedPlan big = plan_clusters_scoped(false, 10000000, 10000000, 0, 0);
    CHECK(big.tiles_a == 78125 && big.tiles_b == 78125 && big.tile_pairs == 6103515625ull);
    CHECK(big.per_launch == kPairsBandTilePairs && big.first_launch == 78125);
    CHECK(launches_cover(big, 0, false) == 1 + (6103515625ull - 78125 + kPairsBandTilePairs - 1) / kPairsBandTilePairs);
    const ClustersScopedPlan bigt = plan_clusters_scoped(true, 10000000, 0, 0, 0);
    CHECK(bigt.tile_pairs == tile_pairs_of(78125) && bigt.first_launch == 78125);
    launches_cover(bigt, 0, false);
    // the knobs and their clamps (clusters_plan.hpp's)
    CHECK(plan_clusters_scoped(true, 1000, 0, 1ull << 40, 0).per_launch == kPairsBandTilePairs);
    CHECK(plan_clusters_scoped(true, 1000, 0, 1ull << 40, 0).first_launch == kPairsBandTilePairs);
    CHECK(plan_clusters_scoped(false, 300, 1000, 2, 0).first_launch == 2 && plan_clusters_scoped(false, 300, 1000, 2, 0).per_launch == 2);
    for (uint64_t knob : {0ull, 1ull, 100ull, 16383ull, 16384ull, 16385ull, 1ull << 20, 1ull << 30, 1ull << 40})
        CHECK(plan_clusters_scoped(false, 300, 1000, 0, knob).ambiguous_cap == clusters_ambiguous_cap(knob));
    CHECK(plan_clusters_scoped(true, 300, 0, 0, 1).ambiguous_cap == 16384);
    CHECK(plan_clusters_scoped(true, 300, 0, 0, 1ull << 40).ambiguous_cap == 1ull << 30);
    // splitting
    for (uint64_t count : {1ull, 2ull, 3ull, 24ull, 1000ull, 16384ull, 65537ull}) split_ends(777, count);
    for (uint64_t launch : {0ull, 1ull, 2ull, 5ull})
        for (uint64_t per_pair : {0ull, 1ull, 8128ull, 16384ull})
            for (uint64_t cap : {0ull, 1ull}) {
                walk(plan_clusters_scoped(true, 380, 0, launch, cap), per_pair);
                walk(plan_clusters_scoped(true, 20000, 0, launch, cap), per_pair);
                walk(plan_clusters_scoped(false, 190, 190, launch, cap), per_pair);
                walk(plan_clusters_scoped(false, 300, 20000, launch, cap), per_pair);
            }
    // the empty joins: tile_pairs == 0 exactly there
    for (uint64_t n : {0ull, 1ull, 2ull, 128ull, 129ull, 5000ull}) {
        CHECK((plan_clusters_scoped(true, n, 77, 0, 0).tile_pairs == 0) == (n < 2));
        for (uint64_t m : {0ull, 1ull, 2ull, 129ull}) {
            CHECK((plan_clusters_scoped(false, n, m, 0, 0).tile_pairs == 0) == (n == 0 || m == 0));
            CHECK((plan_clusters_scoped(false, n, m, 3, 1).tile_pairs == 0) == (n == 0 || m == 0));
        }
    }
    CHECK(plan_clusters_scoped(false, 1, 1, 0, 0).tile_pairs == 1);  // the same single row twice: the caller's to notice
    CHECK(plan_clusters_scoped(false, 0, 500, 0, 0).rows_a == 0 && plan_clusters_scoped(false, 0, 500, 0, 0).rows_b == 500);
    launches_cover(plan_clusters_scoped(false, 0, 500, 0, 0), 0, true);
    launches_cover(plan_clusters_scoped(true, 1, 0, 0, 0), 0, true);
    CHECK(CS_NO_ID == 0xFFFFFFFFu);
    std::printf("clusters scoped plan ok\n");
    return 0;
}
