// pairs_scoped_plan.hpp — the host side of the scoped similar-pairs search (cs_index_similar_pairs_scoped; kernels:
// scan_pairs_scoped.hip): the geometry of the join of two scopes' row lists as plain C++17, no HIP.
// tests/cpp/pairs_scoped_plan_test.cpp walks it on the CPU; index_joins.hip and scan_pairs_scoped.hip only launch what it says.
//
// Both sides are PACKED: list entry i of a scope (its i-th live stored row, ascending) becomes packed row i of an f16 buffer
// of the call's own, in the filter copy's tiled layout.  A side of n live rows is T = ceil(n / 128) packed tiles and
//   packed_bytes = T * 128 * dim * 2        (dim 1024, all of 10M rows: 78,125 tiles, 2.048e10 bytes; size_t throughout).
//
//   same handle        the TRIANGLE of pairs_plan.hpp as it stands: tile_pairs_of(T) tile pairs, tile_pair_of its inverse.
//   different handles  the RECTANGLE of TA x TB tile pairs, numbered row by row:  index(ti, tj) = ti * TB + tj.
//                      The scope with fewer live rows sits on the A side (swapped says that the caller's scope_b did): rows
//                      of the rectangle are then as long as they can be, and an XCD's run of consecutive indices shares
//                      one A tile and reads neighbouring B tiles, as the triangle's does.
// Ranges: T <= 2^25 (a list holds at most 2^32 - 1 rows), so TA * TB < 2^50 and every index, band start and product below
// stays inside 64 bits with room to spare — 6.1e9 tile pairs when both sides hold all of 10M rows.  Either form is launched
// in bands of at most kPairsBandTilePairs consecutive indices, with PairsPlan::xcd_run / band_blocks as the grid.
#pragma once

#include <cstddef>
#include <cstdint>

#include "pairs_plan.hpp"

namespace cs {

// (the numbering itself: read by the plan's test, which checks the inverse below against it)
CS_PAIRS_HD inline uint64_t rect_index_of(uint64_t ti, uint64_t tj, uint64_t tiles_b) { return ti * tiles_b + tj; }
CS_PAIRS_HD inline void rect_pair_of(uint64_t index, uint64_t tiles_b, uint64_t& ti, uint64_t& tj) {
    ti = index / tiles_b;
    tj = index - ti * tiles_b;
}

inline uint64_t packed_tiles_of(uint64_t rows) { return (rows + kPairsTileRows - 1) / kPairsTileRows; }
inline size_t packed_bytes_of(uint64_t tiles, uint32_t dim) { return (size_t)tiles * kPairsTileRows * dim * 2; }

struct PairsScopedPlan {
    bool triangle = true;     // same handle: pairs inside one list
    bool swapped = false;     // rectangle: the caller's scope_b is the A side (it holds fewer live rows)
    uint64_t rows_a = 0, rows_b = 0;    // live rows per side, after the swap (triangle: equal)
    uint64_t tiles_a = 0, tiles_b = 0;  // packed tiles per side
    uint64_t tile_pairs = 0;  // 0: the answer is empty whatever the rows hold, nothing is launched
    uint64_t cand_cap = 0;
    uint64_t bands = 0;

    PairsBand band(uint64_t i) const {
        const uint64_t first = i * kPairsBandTilePairs;
        const uint64_t left = tile_pairs - first;
        return PairsBand{first, left < kPairsBandTilePairs ? left : kPairsBandTilePairs};
    }
    void pair_of(uint64_t index, uint64_t& ti, uint64_t& tj) const {
        if (triangle) tile_pair_of(index, tiles_a, ti, tj);
        else rect_pair_of(index, tiles_b, ti, tj);
    }
};

// live_a / live_b: the lengths of the two lists (same: one list, live_b is not read).  A list of fewer than two rows
// joined with itself, and a join with an empty side, hold no pair: tile_pairs = 0.  (Two different handles that hold the
// same single row hold none either; that takes the rows themselves and is the caller's to notice.)
inline PairsScopedPlan plan_pairs_scoped(bool same, uint64_t live_a, uint64_t live_b, uint32_t max_pairs) {
    PairsScopedPlan p;
    p.triangle = same;
    p.cand_cap = pairs_cand_cap(max_pairs);
    if (same) {
        p.rows_a = p.rows_b = live_a;
        p.tiles_a = p.tiles_b = packed_tiles_of(live_a);
        p.tile_pairs = live_a < 2 ? 0 : tile_pairs_of(p.tiles_a);
    } else {
        p.swapped = live_b < live_a;
        p.rows_a = p.swapped ? live_b : live_a;
        p.rows_b = p.swapped ? live_a : live_b;
        p.tiles_a = packed_tiles_of(p.rows_a);
        p.tiles_b = packed_tiles_of(p.rows_b);
        p.tile_pairs = p.tiles_a * p.tiles_b;  // 0 when a side is empty
    }
    p.bands = (p.tile_pairs + kPairsBandTilePairs - 1) / kPairsBandTilePairs;
    return p;
}

}  // namespace cs
