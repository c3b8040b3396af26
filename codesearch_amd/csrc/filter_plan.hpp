// filter_plan.hpp — the host-side plan of a filter-and-refine search (scan_filter.hip, launch_scan_split): which filter
// kernel scores each phase, in what launch shape, and where the phases end.  Plain C++17, no HIP: tests/cpp/
// filter_plan_test.cpp pins the plan on the CPU, and scan_split_impl only launches what plan_filter returns.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>

namespace cs {

// Phase 0 of the filter searches (scan_filter.hip): tau is still -inf, so the first rows are not filtered at all — every
// one of them is re-scored exactly and folded into the running best-k.  3,072 = a multiple of the filter kernels' 1,024
// row granule that, with the k <= 1,024 carried keys, still sorts as ONE 4,096-key chunk of select_candidates_kernel;
// round 3 used 1,024, which cost one more phase (filter + re-score + select: ~45 us of launches) on a 10M-row index.
constexpr uint32_t kFilterPhase0 = 3072;

// Laboratory knobs of the plan (cs_lab_env: read once by the diagnostic library, scan_filter.hip filter_knobs); the
// defaults are the product's values.
struct FilterKnobs {
    uint32_t int8_max_q = 0;     // CS_FILTER_INT8_MAX_Q: query count up to which the int8 copy is the operand (0: any)
    uint32_t int8_rw_max_q = 0;  // CS_FILTER_INT8_RW_MAX_Q: ... and up to which its resident-query kernel runs (0: 32 tiles)
    bool int8_rq = true;         // CS_FILTER_INT8_RQ=0: above 128 queries at dim 384, rw8<8, 3> instead of the rq8 kernel
    int int8_q2 = 1;             // CS_FILTER_INT8_Q2: two query planes 0 never / 1 long lists of <= 32 queries / 2 <= 64
    int wide_min_q = 129;        // CS_FILTER_WIDE_MIN_Q: query count from which the f16 256 x 256 tile kernel is used
    int rw = 1;                  // CS_FILTER_RW: f16 resident-query kernel 0 off / 1 <= 64 queries / 2 also 128-query tiles
    int growth = 0;              // CS_FILTER_GROWTH: fixed phase growth (1 means 2); 0 = the geometric plan
    uint32_t growth1 = 0;        // CS_FILTER_GROWTH1: fixed growth of the phase right behind phase 0 (> 1)
    double gmax = 0.0;           // CS_FILTER_GMAX: largest ratio between boundaries (> 1; default by k)
    double g1max = 60.0;         // CS_FILTER_G1MAX: the one-round plan's ratio cap
    uint32_t g1_maxq = 4;        // CS_FILTER_G1_MAXQ: query count up to which one round may reach the last row
    double g1_cand = 970.0;      // CS_FILTER_G1_CAND: ... capped at g1_cand / k
    bool int8_rw256 = true;      // CS_FILTER_INT8_RW256=0: 128 instead of 256 resident queries per block (dim 384)
    bool nt = true;              // CS_FILTER_NT=0: default cache policy on the resident-query kernels' corpus stream
    uint32_t phase0_blocks = 96; // CS_FILTER_PHASE0_BLOCKS: refine blocks per query of phase 0 (up to ten queries)
};

enum class FilterKernel : uint8_t {
    None,        // no filter launch: phase 0, or an int8 phase wholly behind the copy's last complete tile
    Q8Tile256,   // score_filter256p_kernel<true>: int8, 256 x 256 tiles, persistent (past 32 resident query tiles)
    Q8Rq,        // score_filter_rq8_kernel<8, 3, false>: dim 384, above 128 queries, eight waves over 256 resident queries
    Q8Rq1,       // score_filter_rq8_kernel<8, 3, true>: the same with one query tile (corpus streamed past the caches)
    Q8Rw,        // score_filter_rw8_kernel<nqt, dim / 128>: int8, resident queries
    Q8Rw2,       // score_filter_rw8_kernel<nqt, dim / 128, true>: the same with the queries in two int8 planes
    F16Rw,       // score_filter_rw_kernel<nqt, dim / 64>: f16 copy, resident queries
    F16Tile256,  // score_filter256p_kernel<false>: f16 copy, 256 x 256 tiles, persistent
    F16Tile128,  // score_filter_kernel: f16 copy, 128 x 128 tiles
};

struct FilterPhase {
    uint64_t lo = 0, hi = 0;          // rows [lo, hi); phase 0 (lo = 0) goes straight to the refine
    FilterKernel kernel = FilterKernel::None;
    uint64_t filter_hi = 0;           // the filter kernel's rows are [lo, filter_hi): int8, up to the copy's last tile
    uint32_t nqt = 0;                 // resident-query kernels: 32-query groups per query tile
    uint32_t qtiles = 0;              // resident-query kernels: query tiles
    uint32_t grid = 0;                // blocks of the filter launch
    uint32_t slots = 0;               // persistent 256 x 256 kernels: (row tile, query tile) slots they walk
    uint64_t tail_lo = 0, tail_hi = 0;  // int8: rows behind the copy's last complete tile (tail_candidates_kernel)
    uint32_t rk_blocks = 0;           // refine blocks per query (rescore_keys_kernel grid.x)
};

// 64 phases: the geometric plan takes at most ten at its default ratios (5.5 and up) over 2^32 rows; with a laboratory
// CS_FILTER_GMAX below ~1.2 the last slot takes every row left.
constexpr uint32_t kMaxFilterPhases = 64;

struct FilterPlan {
    bool use_q8 = false;       // the int8 copy is the filter's operand
    bool two_planes = false;   // ... with the queries in two int8 planes (prep_queries_kernel fills them)
    uint32_t phase0_rows = 0;  // rows of phase 0 (prep_queries_kernel)
    uint32_t nphases = 0;
    FilterPhase phase[kMaxFilterPhases];
};

// (row tiles rounded up to whole XCD octets) x query tiles: split_f16.hpp sh_grid_blocks
inline uint32_t filter_grid_slots(uint32_t mtiles, uint32_t ntiles) { return ((mtiles + 7) / 8) * 8 * ntiles; }

// One block per (query tile, row group) slot of an XCD, at most cus8 blocks: the resident-query kernels' grid.
inline uint32_t filter_resident_grid(uint64_t groups, uint32_t qtiles, int cus8) {
    uint64_t slots = (groups + 7) / 8 * qtiles;  // per XCD
    if (slots > (uint64_t)cus8 / 8) slots = (uint64_t)cus8 / 8;
    if (slots < qtiles) slots = qtiles;
    return (uint32_t)slots * 8;
}

// The plan of one search: nq queries, top-k, over n_rows rows of `dim` (384 / 768 / 1024); q8_rows = rows of a usable
// int8 copy (0: none, or no int8 query workspace), have_query_planes = the two-plane query buffers exist; cus = the
// device's compute units (cu_count, common.hpp).
inline FilterPlan plan_filter(uint32_t dim, uint64_t n_rows, uint32_t nq, uint32_t k, uint64_t q8_rows,
                              bool have_query_planes, int cus, const FilterKnobs& kn) {
    FilterPlan p;
    const uint32_t J = dim / 128;
    // one persistent block per (query tile, row group) slot of an XCD: at most 32 query tiles
    const uint32_t q8_rw_limit = dim <= 768 ? 32u * 128u : 32u * 64u;
    // Measured over 10M x 384, k = 10, 129 / 256 / 512 / 1,000 queries: f16 256 x 256 tiles 2.79 / 2.88 / 5.12 / 8.92 ms,
    // the same tile kernel on int8 2.30 / 2.45 / 4.36 / 7.98 (LDS traffic, not MFMA rate, paces it), the resident-query
    // kernel on int8 1.61 / 1.82 / 3.20 / 5.95 — so the tile kernel only takes what exceeds 32 query tiles.
    const uint32_t q8_rw_max = kn.int8_rw_max_q ? std::min(kn.int8_rw_max_q, q8_rw_limit) : q8_rw_limit;
    // phase 0 re-scores its rows once PER QUERY (L2 traffic nq x rows x dim x 4): 3,072 rows up to 32 queries, 1,024 above
    const uint32_t phase0 = nq <= 32 ? kFilterPhase0 : 1024u;
    // int8 copy: the filter's operand whenever one exists and covers at least one tile behind phase 0
    p.use_q8 = q8_rows > kFilterPhase0 && (!kn.int8_max_q || nq <= kn.int8_max_q);
    // Long lists for up to 32 queries (dim <= 768) take the queries in two int8 planes: a 128 times finer query scale
    // (band ~0.010 instead of ~0.017 for evenly spread vectors: the k-th best of a long list sits where scores are dense,
    // and the band decides how many rows pass) for a second MFMA per step (score_filter_rw8_kernel<.., true>).  The
    // second MFMA is not free even where the kernel streams — same-box A/B over 10M rows: 9 x 200 0.877 -> 0.863 ms,
    // 1 x 200 0.836 -> 0.811, but 8 x 10 0.681 -> 0.712 and 64 x 10 0.81 -> 1.04 — so short lists and more than 32
    // queries keep one plane.  CS_FILTER_INT8_Q2=0: never; =2: whenever the kernel exists (<= 64 queries).
    p.two_planes = p.use_q8 && kn.int8_q2 > 0 && J <= 6 && have_query_planes &&
                   (kn.int8_q2 >= 2 ? nq <= 64 : (nq <= 32 && k >= 48));
    p.phase0_rows = (uint32_t)(n_rows < phase0 ? n_rows : phase0);
    const bool wide = (int)nq >= kn.wide_min_q;
    // resident-query kernel: up to 64 queries always; above that when CS_FILTER_RW=2 (128-query tiles)
    const bool small = kn.rw && (dim == 384 ? (nq <= 64 || (kn.rw >= 2 && (nq + 127) / 128 <= 32))
                                            : nq <= (dim == 768 ? 64u : 32u));
    const int cus8 = cus >= 8 ? cus / 8 * 8 : 256;  // one persistent block per CU (grid rounded down to whole XCD octets)
    // refine blocks per query (blocks past a query's candidate count exit at once): enough that a
    // k = 200 phase (~500 rows per query) is one or two rounds of 32 rows per block
    const uint32_t rk_blocks = nq <= 128 ? 32 : (4096 / nq < 4 ? 4 : 4096 / nq);
    uint64_t done = 0;
    uint64_t phase = p.phase0_rows;  // phase 0: tau = -inf, every row is a candidate
    // A phase that takes the rows scanned from D to g D yields about k (g - 1) candidates per query (each new row beats
    // the k-th best of D exchangeable rows with probability k / D), plus the few inside the margin.  Small growth wins on
    // refine work (re-scoring + sorting grow with it), large growth on launches: a phase is three kernels (filter,
    // re-score, select) and the early ones are launch-bound whatever their size.  Measured over 10M rows (r01-r03):
    // g = 5 from k = 48 on, g = 9 ... 16 below.  Round 4 plans the boundaries as ONE geometric sequence from phase 0 to
    // the last row with the fewest phases whose ratio stays within that growth (5.5 from k = 48, up to 24 below): 10M rows
    // take 5 filter phases at k = 200 (was 6) and 3 at k = 10 (was 4), 1M rows 2 at k = 10.  CS_FILTER_GROWTH / CS_FILTER_GROWTH1 restore fixed growth.
    const bool fixed_growth = kn.growth > 0 || kn.growth1 > 1;
    const uint32_t growth = kn.growth > 0 ? (uint32_t)kn.growth : (k >= 48 ? 4u : 8u);
    double ratio = 0.0;  // planned D_next / D
    if (!fixed_growth && n_rows > phase) {
        // Short lists: a round from D to r D rows brings ~k r candidates times the band's factor (the tail just below tau:
        // exp(z band / sigma) = 3.3 at the 25th best of 175k isotropic rows) into a 4,096-slot buffer — r = 57 overflowed
        // at k = 25 and fell back to the exact scan (profiles/r04_filter_gmax_ab.log); 24, capped by 900 / k, keeps a
        // factor of 4.5 in hand and lets 1M rows take two rounds instead of three (153 -> 138 us at k = 10)
        // ... except where ONE round reaches the last row: up to four queries over at most min(60, 970 / k) x 3,072 rows expect
        // ~k r 3.3 <= 3,200 candidates, and should the buffer overflow after all, the exact rerun behind it costs what a
        // streaming scan of so few rows costs (~100 us), not the 2.2 ms of a 10M-row corpus: one query over 100,000 rows 77 -> 65 us
        // at k = 10, 84 -> 74 at k = 20, 86 -> 78 at k = 25.  (Five to ten queries gain 5 % at 100,000 rows and lose 7 % at
        // 184,000 — their candidates multiply the refine: they keep the capped plan; profiles/r04_filter_one_round_ab.log.)
        const double g1 = std::min(kn.g1max, kn.g1_cand / (double)k);  // 60 up to k = 16, 38.8 at k = 25, no more than the cap of 24 from k = 40
        const bool one_round = nq <= kn.g1_maxq && g1 > 24.0 && (double)n_rows <= g1 * (double)phase;
        const double gshort = one_round ? g1 : std::min(24.0, 900.0 / (double)k);
        const double gmax = kn.gmax > 1.0 ? kn.gmax : (k >= 48 ? 5.5 : gshort), span = (double)n_rows / (double)phase;
        const double nph = std::ceil(std::log(span) / std::log(gmax) - 1e-9);
        ratio = std::pow(span, 1.0 / (nph < 1.0 ? 1.0 : nph));
    }
    do {
        FilterPhase& f = p.phase[p.nphases++];
        f.lo = done;
        f.hi = done + phase;
        f.filter_hi = f.hi;
        const bool first = f.lo == 0;  // phase 0 goes straight to the refine (rescore_keys_kernel, first_rows)
        if (f.hi > f.lo && !first) {
            if (p.use_q8) {
                const uint64_t q_hi = f.hi < q8_rows ? f.hi : q8_rows;  // lo is a multiple of 1024
                f.filter_hi = q_hi;
                if (q_hi > f.lo && nq > q8_rw_max) {
                    f.kernel = FilterKernel::Q8Tile256;
                    f.slots = filter_grid_slots((uint32_t)((q_hi - f.lo + 255) / 256), (nq + 255) / 256);
                    f.grid = std::min<uint32_t>(f.slots, (uint32_t)cus8);  // a multiple of 8: a block stays on its XCD slot
                } else if (q_hi > f.lo && J == 3 && nq > 128 && kn.int8_rq) {
                    // many queries at dim 384: eight waves over 256 resident queries, corpus fragments through registers
                    f.nqt = 8;
                    f.qtiles = (nq + 255) / 256;
                    f.kernel = f.qtiles == 1 ? FilterKernel::Q8Rq1 : FilterKernel::Q8Rq;
                    f.grid = filter_resident_grid(((q_hi - f.lo) / 128 + 1) / 2, f.qtiles, cus8);  // 256-row units
                } else if (q_hi > f.lo) {
                    // above 128 queries at dim 384: 256 resident queries per block — half the query tiles re-reading the
                    // corpus through L2 (1,000 queries over 10M rows: 7.21 -> 5.95 ms; 129: 1.97 -> 1.61); "0" = A/B
                    const uint32_t per =
                        nq <= 32 ? 32 : (nq <= 64 || J > 6) ? 64 : (J == 3 && kn.int8_rw256 && nq > 128) ? 256 : 128;
                    f.kernel = per <= 64 && p.two_planes ? FilterKernel::Q8Rw2 : FilterKernel::Q8Rw;
                    f.nqt = per / 32;
                    f.qtiles = (nq + per - 1) / per;
                    f.grid = filter_resident_grid((q_hi - f.lo) / 128, f.qtiles, cus8);
                }
                f.tail_lo = f.lo > q8_rows ? f.lo : q8_rows;
                f.tail_hi = f.hi > f.tail_lo ? f.hi : f.tail_lo;  // fewer than 128 rows behind the last complete tile
            } else if (small) {
                const uint32_t per = nq <= 32 ? 32 : nq <= 64 ? 64 : 128;
                f.kernel = FilterKernel::F16Rw;
                f.nqt = per / 32;
                f.qtiles = (nq + per - 1) / per;
                f.grid = filter_resident_grid((f.hi - f.lo + 127) / 128, f.qtiles, cus8);  // one row group per tile at most
            } else if (wide) {
                f.kernel = FilterKernel::F16Tile256;
                f.slots = filter_grid_slots((uint32_t)((f.hi - f.lo + 255) / 256), (nq + 255) / 256);
                f.grid = std::min<uint32_t>(f.slots, ((uint32_t)cus + 7) / 8 * 8);  // a multiple of 8: a block stays on its XCD slot
            } else {
                f.kernel = FilterKernel::F16Tile128;
                f.grid = filter_grid_slots((uint32_t)((f.hi - f.lo + 127) / 128), (nq + 127) / 128);
            }
        }
        done = f.hi;
        // refine: exact keys in place (each query's rows spread over rk_blocks CUs), then the select
        // phase 0 of a few queries: its 3,072 rows in ONE round of 32 rows per block (96 blocks per query instead of three
        // rounds on 32: the phase is a dependent launch in front of every filter search, 12 -> 7 us for one query)
        f.rk_blocks = (first && nq * kn.phase0_blocks <= 1024 && kn.phase0_blocks > rk_blocks) ? kn.phase0_blocks : rk_blocks;
        if (fixed_growth) {
            // (round 3's rule: the phase right behind phase 0 takes 16 x the rows seen for short lists, growth + 1 otherwise)
            const uint32_t growth1 = kn.growth1 > 1 ? kn.growth1 : (k < 48 && kn.growth <= 0 ? 16u : growth + 1);
            phase = done * (first ? growth1 - 1 : growth);
        } else {
            // next boundary of the geometric plan, on the filter kernels' 1,024-row granule
            uint64_t next = (uint64_t)std::ceil((double)done * ratio);
            next = (next + 1023) / 1024 * 1024;
            if (next <= done) next = done + 1024;
            phase = next - done;
            if ((double)(n_rows - done) < (double)phase * 1.25) phase = n_rows - done;  // no sliver of a last phase
        }
        if (phase > n_rows - done || p.nphases == kMaxFilterPhases - 1) phase = n_rows - done;
    } while (done < n_rows);
    return p;
}

}  // namespace cs
