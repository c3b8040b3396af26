// pairs_plan_test.cpp — the host plan of the similar-pairs search (codesearch_amd/csrc/pairs_plan.hpp) on the CPU, a
// stand-alone program: tests/test_similar_pairs_host.py builds it once plain and once under AddressSanitizer + UBSan.
//   * tile_pair_of is a bijection onto {ti <= tj}, exhaustively for T = 1 .. 300, in the triangle's row order;
//   * at T = 78,125 (10M rows; 3.05e9 tile pairs) the first and last index of every 1,000th row of the triangle and the last
//     index overall map where the closed form says — the sizes at which an uncorrected float sqrt goes wrong;
//   * the bands cover every tile pair exactly once, none exceeds the cap, and the filter's grid covers a band exactly once;
//   * cand_cap has the formula's value at max_pairs = 1, 65,536 and CS_MAX_PAIRS.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../codesearch_amd/csrc/pairs_plan.hpp"
#include "../../include/codesearch_gpu.h"

using namespace cs;

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                       \
        }                                                                       \
    } while (0)

// the closed form of pairs_plan.hpp's header: row ti starts behind the ti rows of T, T - 1, ... pairs before it
static uint64_t index_of(uint64_t ti, uint64_t tj, uint64_t T) { return ti * T - (ti ? ti * (ti - 1) / 2 : 0) + (tj - ti); }

static void bijection_small() {
    for (uint64_t T = 1; T <= 300; ++T) {
        uint64_t idx = 0;
        for (uint64_t ti = 0; ti < T; ++ti)
            for (uint64_t tj = ti; tj < T; ++tj, ++idx) {
                uint64_t a = ~0ull, b = ~0ull;
                tile_pair_of(idx, T, a, b);
                CHECK(a == ti && b == tj);
                CHECK(index_of(ti, tj, T) == idx);
            }
        CHECK(idx == tile_pairs_of(T));
    }
}

static void large_triangle() {
    const uint64_t T = 78125;
    const uint64_t P = tile_pairs_of(T);
    CHECK(P == 3051796875ull);
    uint64_t a = 0, b = 0;
    uint64_t first = 0;  // index of row ti's diagonal pair
    for (uint64_t ti = 0; ti < T; ++ti) {
        if (ti % 1000 == 0 || ti == T - 1) {
            tile_pair_of(first, T, a, b);
            CHECK(a == ti && b == ti);
            tile_pair_of(first + (T - ti) - 1, T, a, b);
            CHECK(a == ti && b == T - 1);
            if (first) {  // the pair before a row's first is the previous row's last
                tile_pair_of(first - 1, T, a, b);
                CHECK(a == ti - 1 && b == T - 1);
            }
        }
        first += T - ti;
    }
    CHECK(first == P);
    tile_pair_of(P - 1, T, a, b);
    CHECK(a == T - 1 && b == T - 1);
    tile_pair_of(0, T, a, b);
    CHECK(a == 0 && b == 0);
}

static void bands_cover(uint64_t rows, uint32_t max_pairs) {
    const PairsPlan p = plan_pairs(rows, max_pairs, 256);
    CHECK(p.tiles == (rows + 127) / 128);
    CHECK(p.tile_pairs == p.tiles * (p.tiles + 1) / 2);
    CHECK(p.cand_cap == 2ull * max_pairs + 4096);
    CHECK(p.refine_blocks >= 1 && p.refine_blocks <= 8u * 256u);
    uint64_t next = 0;
    for (uint64_t i = 0; i < p.bands; ++i) {
        const PairsBand b = p.band(i);
        CHECK(b.first == next);
        CHECK(b.count >= 1 && b.count <= kPairsBandTilePairs);
        next += b.count;
        // the grid of a band: block x -> (x & 7) * run + (x >> 3), kept when < count — every pair of the band once
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
    }
    CHECK(next == p.tile_pairs);
    CHECK(p.bands == (p.tile_pairs + kPairsBandTilePairs - 1) / kPairsBandTilePairs);
}

int main() {
    bijection_small();
    large_triangle();
    for (uint64_t rows : {0ull, 1ull, 2ull, 127ull, 128ull, 129ull, 1000ull, 100000ull, 185344ull, 185345ull, 1000000ull, 10000000ull})
        for (uint32_t mp : {1u, 65536u, (uint32_t)CS_MAX_PAIRS}) bands_cover(rows, mp);
    CHECK(plan_pairs(0, 1, 256).bands == 0 && plan_pairs(0, 1, 256).tile_pairs == 0);
    CHECK(plan_pairs(1000, 1, 256).tile_pairs == 36 && plan_pairs(1000, 1, 256).bands == 1);
    CHECK(plan_pairs(1000000, 1, 256).bands == 30);  // 7,813 tiles, 30.5M tile pairs
    CHECK(pairs_cand_cap(1) == 4098 && pairs_cand_cap(65536) == 135168 && pairs_cand_cap(CS_MAX_PAIRS) == 8392704);
    CHECK(CS_MAX_PAIRS == 1u << 22 && CS_PAIRS_ALL == 0 && CS_PAIRS_OTHER_GROUP == 1);
    CHECK(pairs_refine_blocks(0, 256) == 1 && pairs_refine_blocks(9, 256) == 2 && pairs_refine_blocks(1u << 22, 256) == 2048);
    std::printf("pairs plan ok\n");
    return 0;
}
