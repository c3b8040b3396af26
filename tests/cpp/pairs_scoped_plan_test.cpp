// pairs_scoped_plan_test.cpp — the host plan of the scoped similar-pairs search (codesearch_amd/csrc/pairs_scoped_plan.hpp)
// on the CPU, a stand-alone program: tests/test_similar_pairs_scoped_host.py builds it once plain and once under
// AddressSanitizer + UBSan.
//   * the rectangle's numbering and its inverse, exhaustively for TA, TB in 1 .. 40;
//   * at TA = TB = 78,125 (both sides all of 10M rows; 6.1e9 tile pairs) the first and last index of sampled rows;
//   * the bands of both forms cover every index exactly once, none exceeds the cap, the grid covers a band exactly once;
//   * which side sits where, the empty joins, the packed buffers' bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codesearch_amd/csrc/pairs_scoped_plan.hpp"
#include "../../include/codesearch_gpu.h"

using namespace cs;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

static void rectangle_small() {
    for (uint64_t TA = 1; TA <= 40; ++TA)
        for (uint64_t TB = 1; TB <= 40; ++TB) {
            uint64_t idx = 0;
            for (uint64_t ti = 0; ti < TA; ++ti)
                for (uint64_t tj = 0; tj < TB; ++tj, ++idx) {
                    uint64_t a = ~0ull, b = ~0ull;
                    rect_pair_of(idx, TB, a, b);
                    CHECK(a == ti && b == tj);
                    CHECK(rect_index_of(ti, tj, TB) == idx);
                }
            CHECK(idx == TA * TB);
        }
}

static void rectangle_large() {
    const uint64_t T = 78125;
    CHECK(T * T == 6103515625ull);
    uint64_t a = 0, b = 0;
    std::vector<uint64_t> sampled;
    for (uint64_t ti = 0; ti < T; ti += 1000) sampled.push_back(ti);
    sampled.push_back(T - 1);
    for (uint64_t ti : sampled) {
        rect_pair_of(ti * T, T, a, b);
        CHECK(a == ti && b == 0);
        rect_pair_of(ti * T + T - 1, T, a, b);
        CHECK(a == ti && b == T - 1);
        if (ti) {
            rect_pair_of(ti * T - 1, T, a, b);
            CHECK(a == ti - 1 && b == T - 1);
        }
    }
    rect_pair_of(T * T - 1, T, a, b);
    CHECK(a == T - 1 && b == T - 1);
}

static void bands_cover(const PairsScopedPlan& p, uint32_t max_pairs) {
    CHECK(p.cand_cap == 2ull * max_pairs + 4096);
    CHECK(p.bands == (p.tile_pairs + kPairsBandTilePairs - 1) / kPairsBandTilePairs);
    uint64_t next = 0;
    for (uint64_t i = 0; i < p.bands; ++i) {
        const PairsBand b = p.band(i);
        CHECK(b.first == next);
        CHECK(b.count >= 1 && b.count <= kPairsBandTilePairs);
        next += b.count;
        const uint64_t run = PairsPlan::xcd_run(b.count), blocks = PairsPlan::band_blocks(b.count);
        CHECK(blocks == 8 * run && blocks >= b.count && blocks < b.count + 8 && blocks <= 0xFFFFFFFFull);
        if (b.count <= 4096) {
            std::vector<int> seen(b.count, 0);
            for (uint64_t x = 0; x < blocks; ++x) {
                const uint64_t in_band = (x & 7) * run + (x >> 3);
                if (in_band < b.count) seen[in_band]++;
            }
            for (int s : seen) CHECK(s == 1);
        }
        // the band's first and last index land inside the join
        for (uint64_t idx : {b.first, b.first + b.count - 1}) {
            uint64_t ti = ~0ull, tj = ~0ull;
            p.pair_of(idx, ti, tj);
            CHECK(ti < p.tiles_a && tj < p.tiles_b);
            if (p.triangle) CHECK(ti <= tj);
            else CHECK(rect_index_of(ti, tj, p.tiles_b) == idx);
        }
    }
    CHECK(next == p.tile_pairs);
}

int main() {
    rectangle_small();
    rectangle_large();
    const uint64_t sizes[] = {0, 1, 2, 127, 128, 129, 300, 1000, 100000, 1000000, 10000000};
    for (uint32_t mp : {1u, 65536u, (uint32_t)CS_MAX_PAIRS})
        for (uint64_t na : sizes) {
            const PairsScopedPlan t = plan_pairs_scoped(true, na, 12345, mp);
            CHECK(t.triangle && !t.swapped && t.rows_a == na && t.rows_b == na && t.tiles_a == (na + 127) / 128 && t.tiles_b == t.tiles_a);
            CHECK(t.tile_pairs == (na < 2 ? 0 : tile_pairs_of(t.tiles_a)));
            // the triangle of a scope is the unscoped plan's for as many stored rows
            if (na >= 2) CHECK(t.tile_pairs == plan_pairs(na, mp, 256).tile_pairs && t.bands == plan_pairs(na, mp, 256).bands);
            bands_cover(t, mp);
            for (uint64_t nb : sizes) {
                const PairsScopedPlan r = plan_pairs_scoped(false, na, nb, mp);
                CHECK(!r.triangle && r.swapped == (nb < na));
                CHECK(r.rows_a == (na < nb ? na : nb) && r.rows_b == (na < nb ? nb : na));  // the smaller scope on the A side
                CHECK(r.tiles_a == (r.rows_a + 127) / 128 && r.tiles_b == (r.rows_b + 127) / 128);
                CHECK(r.tile_pairs == r.tiles_a * r.tiles_b);
                CHECK((r.tile_pairs == 0) == (na == 0 || nb == 0));
                bands_cover(r, mp);
            }
        }
    // the empty joins launch nothing
    CHECK(plan_pairs_scoped(true, 0, 0, 1).bands == 0 && plan_pairs_scoped(true, 1, 1, 1).bands == 0);
    CHECK(plan_pairs_scoped(false, 0, 500, 1).bands == 0 && plan_pairs_scoped(false, 500, 0, 1).bands == 0);
    CHECK(plan_pairs_scoped(true, 2, 2, 1).tile_pairs == 1 && plan_pairs_scoped(false, 129, 1, 1).tile_pairs == 2);
    CHECK(plan_pairs_scoped(false, 129, 1, 1).swapped && !plan_pairs_scoped(false, 1, 129, 1).swapped);
    // 10M rows on both sides: 6.1e9 tile pairs in 5,821 bands; a 10 % scope of 1M rows is 1 % of the store's triangle
    const PairsScopedPlan big = plan_pairs_scoped(false, 10000000, 10000000, 65536);
    CHECK(big.tile_pairs == 6103515625ull && big.bands == 5821);
    CHECK(plan_pairs_scoped(true, 100000, 0, 65536).tile_pairs == tile_pairs_of(782));
    CHECK(tile_pairs_of(782) * 99 < tile_pairs_of(7813) && tile_pairs_of(7813) < tile_pairs_of(782) * 100);
    // packed buffers: whole tiles, 2 bytes per element
    CHECK(packed_tiles_of(0) == 0 && packed_tiles_of(1) == 1 && packed_tiles_of(128) == 1 && packed_tiles_of(129) == 2);
    CHECK(packed_bytes_of(1, 384) == 128u * 384u * 2u && packed_bytes_of(78125, 1024) == 20480000000ull);
    std::printf("pairs scoped plan ok\n");
    return 0;
}
