// pairs_plan.hpp — the host side of the similar-pairs search (cs_index_similar_pairs; kernels: scan_pairs.hip): the
// geometry of the self-join as plain C++17, no HIP.  tests/cpp/pairs_plan_test.cpp walks it on the CPU; index_joins.hip and
// scan_pairs.hip only launch what it says.
//
// The corpus is T = ceil(stored_rows / 128) tiles of 128 rows (the tiles of the f16 filter copy).  The join scores every tile
// pair (ti, tj) with ti <= tj — T (T + 1) / 2 of them, one block each — numbered row by row through the upper triangle:
//   index(ti, tj) = ti T - ti (ti - 1) / 2 + (tj - ti)            row ti holds T - ti pairs, the diagonal one first.
// The pairs are launched in BANDS of at most kPairsBandTilePairs consecutive indices: the host reads the candidate counter
// between bands and stops at the first overflow, so no single kernel runs longer than a band and a bound that is far too
// low fails after one band instead of after the whole triangle.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define CS_PAIRS_HD __host__ __device__
#else
#define CS_PAIRS_HD
#endif

namespace cs {

constexpr uint32_t kPairsTileRows = 128;
// Tile pairs one launch may score.  A tile pair is 2 * 128 * 128 * dim f16 FLOP (1.26e7 at dim 384, 3.36e7 at 1024), so a
// full band is 1.3e13 / 3.5e13 FLOP: 13 / 35 ms if the filter sustains 1e15 FLOP/s, twice that at half the rate.  An
// ESTIMATE from the arithmetic, not a measurement: "tens of milliseconds" is all it is meant to guarantee.
constexpr uint64_t kPairsBandTilePairs = 1ull << 20;
constexpr uint32_t kPairsRefineThreads = 256;  // eight half-waves, one candidate pair each per round

// Candidate pairs the device holds for a call that may return max_pairs pairs.
CS_PAIRS_HD inline uint64_t pairs_cand_cap(uint32_t max_pairs) { return 2ull * max_pairs + 4096ull; }

CS_PAIRS_HD inline uint64_t tile_pairs_of(uint64_t tiles) { return tiles * (tiles + 1) / 2; }

// index -> (ti, tj), exact in 64-bit integers for T <= 78,125 (3.05e9 pairs) and far beyond: counted from the END of the
// triangle the rows hold 1, 2, 3 ... pairs, so with rem = P - 1 - index the row is the largest m with m (m + 1) / 2 <= rem.
// The double sqrt gives m to within one (8 rem + 1 < 2^53 is exact in a double; the root is rounded once); the two loops
// settle it in integers.
CS_PAIRS_HD inline void tile_pair_of(uint64_t index, uint64_t tiles, uint64_t& ti, uint64_t& tj) {
    const uint64_t rem = tile_pairs_of(tiles) - 1 - index;
    uint64_t m = (uint64_t)((sqrt((double)(8 * rem + 1)) - 1.0) * 0.5);
    while (m * (m + 1) / 2 > rem) --m;
    while ((m + 1) * (m + 2) / 2 <= rem) ++m;
    const uint64_t p = rem - m * (m + 1) / 2;  // position in the row, counted from its end
    ti = tiles - 1 - m;
    tj = tiles - 1 - p;
}

struct PairsBand {
    uint64_t first;  // index of the band's first tile pair
    uint64_t count;  // tile pairs in it, 1 .. kPairsBandTilePairs
};

struct PairsPlan {
    uint64_t tiles = 0;       // T
    uint64_t tile_pairs = 0;  // T (T + 1) / 2
    uint64_t cand_cap = 0;    // candidate pairs the device holds
    uint64_t bands = 0;       // launches of the filter
    uint32_t refine_blocks = 0;  // grid of the refine for a full candidate buffer (a grid-stride kernel: an upper bound)

    PairsBand band(uint64_t i) const {
        const uint64_t first = i * kPairsBandTilePairs;
        const uint64_t left = tile_pairs - first;
        return PairsBand{first, left < kPairsBandTilePairs ? left : kPairsBandTilePairs};
    }
    // the filter's grid for a band: every XCD (block index mod 8) walks its own run of `xcd_run` consecutive tile pairs
    static uint64_t xcd_run(uint64_t count) { return (count + 7) / 8; }
    static uint64_t band_blocks(uint64_t count) { return 8 * xcd_run(count); }
};

// Grid of the refine for n candidates: one half-wave per candidate per round, at most eight blocks per CU.
inline uint32_t pairs_refine_blocks(uint64_t n, int cu_count) {
    const uint64_t per = kPairsRefineThreads / 32;
    const uint64_t want = (n + per - 1) / per;
    const uint64_t most = 8ull * (uint64_t)(cu_count > 0 ? cu_count : 1);
    const uint64_t b = want < most ? want : most;
    return (uint32_t)(b ? b : 1);
}

inline PairsPlan plan_pairs(uint64_t stored_rows, uint32_t max_pairs, int cu_count) {
    PairsPlan p;
    p.tiles = (stored_rows + kPairsTileRows - 1) / kPairsTileRows;
    p.tile_pairs = tile_pairs_of(p.tiles);
    p.cand_cap = pairs_cand_cap(max_pairs);
    p.bands = (p.tile_pairs + kPairsBandTilePairs - 1) / kPairsBandTilePairs;
    p.refine_blocks = pairs_refine_blocks(p.cand_cap, cu_count);
    return p;
}

}  // namespace cs
