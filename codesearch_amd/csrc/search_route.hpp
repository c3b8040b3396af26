// search_route.hpp — the route of an index search (index.hip run_search): whether it wants the filter, then which path
// answers it, where its queries are read from and whether a prime pass runs in front of the streaming scan.  Plain C++17,
// no HIP: tests/cpp/search_route_test.cpp pins the routes on the CPU, and run_search only launches what plan_route returns.
#pragma once

#include <cstdint>

#include "../../include/codesearch_gpu.h"  // CS_ROUTE_*
#include "filter_plan.hpp"                 // kFilterPhase0

namespace cs {

// The route's thresholds, one set per index (index.hip fills it from the environment at cs_index_create).
struct RouteKnobs {
    int filter_min_q = 2;  // query count from which the f16 filter + exact refine path is used
    uint32_t single_filter_min_k = 100;  // ... and one query too from this k on, over >= 2M rows (0 = never)
    // One query: CS_ROUTE_COST (default) takes the filter over >= single_int8_min_rows rows whenever the int8 copy serves
    // (same bits, 0.66 vs 2.16 ms over 10M x 384 at k = 10: the filter streams a quarter of the bytes), and from
    // single_filter_min_k on over >= single_filter_min_rows rows with the f16 copy; CS_ROUTE_STREAM always runs the f32 streaming scan (the north-star
    // kernel: bench.py selects it for `value`); CS_ROUTE_FILTER takes the filter whenever a copy can serve.
    int single_route = CS_ROUTE_COST;
    uint64_t single_filter_min_rows = 2000000;  // ... with the f16 copy (and k >= single_filter_min_k)
    // ... with the int8 copy: the measured crossover of the two routes, which depends on the list length because the
    // filter's round plan does (filter_plan.hpp: growth up to 24 - one round up to 60 x 3,072 rows - below k = 48, 5.5 from
    // there on).  profiles/r04_route_crossover_by_k.log, us per search, stream / filter: k = 10: 20k rows 54 / 57, 35k 63 / 58,
    // 100k 83 / 65, 184k 105 / 72; k = 25: 35k 71 / 63, 100k 104 / 86; k = 40: 200k 158 / 102 — k = 50: 150k 97 / 114, 300k 129 / 127,
    // 400k 150 / 131; k = 75: 300k 141 / 135; k = 99: 300k 142 / 141.  (Round 4's first figure, 150,000 rows for every k, was
    // taken before the phase plan and the one-round phase 0.)
    uint64_t single_int8_min_rows = 32768;        // k < 48 (CS_FILTER_SINGLE_MIN_ROWS)
    uint64_t single_int8_min_rows_long = 300000;  // k >= 48 (CS_FILTER_SINGLE_MIN_ROWS_LONG)
    uint64_t few_queries_min_rows = 40000;        // two or three queries: rows from which they take the filter (CS_FILTER_FEW_MIN_ROWS) ...
    uint64_t few_queries_min_rows_short = 16384;  // ... with k <= 16 (both follow CS_FILTER_FEW_MIN_ROWS when it is set)
    uint64_t single_batched_max_rows = 1024;  // ... and one query over at most this many rows (0 = never; CS_SINGLE_BATCHED_MAX_ROWS)
    // primed streaming scan (scan.hip PRIME mode): from this k and this many rows on, a pass over
    // the first prime_rows rows bounds the list inserts of the full scan
    // (measured, 1 query x 384-d: 10M rows k=10 2.37 -> 2.31 ms, k=200 2.62 -> 2.41 ms; 1M rows
    // k=200 382 -> 279 us).  prime_rows 0 = n_rows / 256 clamped to [4096, 16384]; prime_min_rows 0 =
    // 500,000 rows below k = 48 and 100,000 from there on.
    uint32_t prime_min_k = 1;
    uint64_t prime_min_rows = 0, prime_rows = 0;
    // scoped searches through the int8 filter (scoped_filter_plan.hpp scoped_wants_filter): the filter phases may
    // stream at most this many rows per live row of the scope, by query count (CS_SCOPE_FILTER_MAX_SPAN sets all three).
    // Measured over 10M x 384 (profiles/scoped_filter_10m.jsonl), filter / gathered ms at span 2, 4, 10:
    // one query, k = 10: 0.66 / 1.19, 0.66 / 0.63, 0.63 / 0.29; k = 200: 0.77 / 1.24, 0.75 / 0.69, 0.72 / 0.34 — ahead at 2,
    // behind at 4; nine variants, k = 200: 0.87 / 4.33, 0.87 / 2.36, 0.91 / 1.12 — ahead at every measured span (the
    // gathered scan makes three passes, the filter one).  Two to eight queries were not measured: 4 is the byte
    // break-even of one gathered pass (1 B per element streamed against 4 B), reasoning only.
    double scope_span_single = 2.0, scope_span_few = 4.0, scope_span_many = 10.0;
    double scope_filter_max_span(uint32_t nq) const { return nq == 1 ? scope_span_single : nq < 9 ? scope_span_few : scope_span_many; }
};

// One search as the route sees it.
struct SearchShape {
    uint32_t nq = 1, k = 1, dim = 0;
    uint64_t n_rows = 0;
    int cus = 256;               // the device's compute units
    bool normed = false;         // row norms cover every row (the batched paths need them)
    bool use_split = false;      // the index keeps filter copies (split_scan_supported(dim), CS_INDEX_SPLIT)
    bool batched = false;        // batched_supported(dim): the exact-f32 MFMA path exists
    bool prime = false;          // scan_prime_supported(dim): the prime pass exists, and the scan keeps its queries in registers
    bool pinned = false;         // the queries are in pinned host memory and the device query buffer is empty (host-buffer API)
    uint64_t stream_blocks = 0;  // plan_scan's blocks x passes
};

// Stream: the f32 streaming scan + merge (scan.hip), with or without the prime pass; Filter: the filter + exact refine
// (scan_filter.hip) on the copy index.hip obtained; BatchedExact: the exact-f32 MFMA batched path (scan_mfma.hip).
enum class SearchPath : uint8_t { Stream, Filter, BatchedExact };

enum class QuerySource : uint8_t {
    Device,        // the caller's device buffer
    PrepPinned,    // the filter's prep kernel reads the pinned buffer and fills the device buffer
    StreamPinned,  // the streaming scan reads the pinned buffer directly
    Copy,          // one H2D copy of the pinned buffer into the device buffer first
};

struct SearchRoute {
    SearchPath path = SearchPath::Stream;
    QuerySource queries = QuerySource::Device;
    uint64_t prime_rows = 0;  // > 0: a prime pass over the first prime_rows rows (Stream only)
};

// Per-wave list capacity of the streaming scan: a power of two >= k, >= 64.
inline uint32_t kpad_for(uint32_t k) {
    uint32_t p = 64;
    while (p < k) p <<= 1;
    return p;
}

constexpr uint32_t kScanWaves = 4;  // waves per block of the streaming scan (scan.hip kBlock / 64)

// Prime pass geometry.  The bound is the k-th largest of W wave maxima, so W must exceed k by a
// good factor and every wave should see a few tiles: up to k = 256 one block per CU (W <= 1024
// waves); above, four per CU (W <= 4096, the most keys the selecting block's LDS holds) — with
// W = 1024 a k = 1024 bound is the smallest of all maxima, a third of the rows pass it and the scan
// takes 4.9 ms instead of 2.5.  Never more blocks than kpad (waves = 4 * blocks <= 4 * kpad).
inline uint32_t prime_block_cap(uint32_t k, int num_cus) {
    const uint32_t kpad = kpad_for(k);
    uint32_t cap = (uint32_t)num_cus * (k > 256 ? 4u : 1u);
    if (cap > 1024) cap = 1024;
    return cap > kpad ? kpad : cap;
}

// Rows of the prime sample: the caller's default, raised to 32 rows per wave when k > 256.
inline uint64_t prime_sample_rows(uint64_t default_rows, uint32_t k, int num_cus) {
    if (k <= 256) return default_rows;
    const uint64_t want = (uint64_t)prime_block_cap(k, num_cus) * kScanWaves * 32;
    return want > default_rows ? want : default_rows;
}

// Rows the prime pass samples: RouteKnobs::prime_rows, or n_rows / 256 on whole 64-row units clamped to [4,096, 8,192] up to
// k = 16 and to [4,096, 16,384] above, raised to prime_sample_rows when k > 256 and n_rows is at least four times that.
inline uint64_t prime_rows_for(const RouteKnobs& kn, uint64_t n_rows, uint32_t k, int cus) {
    if (kn.prime_rows) return kn.prime_rows;
    uint64_t rows = (n_rows / 256) & ~(uint64_t)63;
    // short lists need fewer wave maxima for a useful bound: 8,192 rows (512 waves of 16) up to k = 16 — over 10M
    // rows the pass costs 18 instead of 26 us and the scan the same (k = 10: 2,122 -> 2,114 us; k = 64 and 99 lose
    // 5 and 17 us with the smaller sample and keep 16,384)
    const uint64_t cap = k <= 16 ? 8192 : 16384;
    rows = rows < 4096 ? 4096 : (rows > cap ? cap : rows);
    const uint64_t big = prime_sample_rows(rows, k, cus);  // k > 256: more waves, 32 rows each
    return n_rows >= 4 * big ? big : rows;
}

// Step 1: does this search want the filter?  q8_serves: the int8 copy serves as the filter's operand (index.hip q8_serves,
// read before the workspace folds newly reported overflows into strikes).  Only then does index.hip look for a filter
// copy: the int8 one when it serves and its query planes fit, else the f16 one, built on demand.
inline bool route_wants_filter(const RouteKnobs& kn, const SearchShape& s, bool q8_serves) {
    if (!s.use_split || !s.normed) return false;
    const uint32_t nq = s.nq, k = s.k;
    const uint64_t n = s.n_rows;
    // One query normally stays on the exact f32 streaming scan (the north-star kernel).  With a long list over a
    // multi-million-row index — the reference's own retrieval_limit (100 or 200) when a search has no query variants —
    // the filter + refine path is taken instead: same bits, 1.40 vs 2.36 ms at k = 200 over 10M x 384, because
    // the scan's list inserts need a second block per CU there and the filter reads half the bytes.
    // ... and over a corpus of the reference's own size (hundreds of chunks) the batched path — prep, direct scoring of
    // every row, select: three small launches, no filter involved below a candidate buffer's worth of rows — answers one
    // query faster than the streaming scan's per-wave lists do (592 rows: 30 vs 41 us; 1,000: 33 vs 46; from 2,000
    // rows on the scan is ahead: 43 vs 48 us).
    const bool single_filter =
        nq == 1 && kn.single_route != CS_ROUTE_STREAM &&
        (kn.single_route == CS_ROUTE_FILTER ||
         (q8_serves && n >= (k < 48 ? kn.single_int8_min_rows : kn.single_int8_min_rows_long)) ||
         (n >= kn.single_filter_min_rows && kn.single_filter_min_k && k >= kn.single_filter_min_k));
    // (First measurement, round 4:) two to four queries over a corpus between one phase 0 and ~50,000 rows: the streaming scan (one pass per query
    // tile) is ahead of the filter's fixed rounds (profiles/r04_batched_route_by_size.log, us per search at nq = 2, k = 25,
    // filter / stream: 2,000 rows 37 / 45; 5,000 63 / 45; 20,000 71 / 60; 100,000 97 / 117); from five queries on the filter
    // wins at every size (9 x 200: 41 ... 277 us against 81 ... 600 on the exact-f32 MFMA path).
    // Re-measured behind the one-round phase 0 and the one-round plan of small corpora (profiles/r04_few_queries_crossover.log,
    // us per search, stream / filter): FOUR queries are ahead on the filter from 5,000 rows on (k = 10: 5k 63 / 54, 20k 78 / 61,
    // 50k 119 / 67; k = 25: 5k 64 / 58, 50k 95 / 76); TWO stream up to ~16,000 rows with a short list (k = 10: 10k 47 / 56,
    // 20k 66 / 61) and up to ~40,000 rows above (k = 25: 20k 60 / 65, 35k 66 / 69, 50k 82 / 73), and THREE cost the streaming
    // scan what two do (one pass: 5k rows 44 / 55, 10k 48 / 57, 20k at k = 25 60 / 66; four take a second pass: 63), so they
    // follow two.
    const uint64_t few_min = k <= 16 ? kn.few_queries_min_rows_short : kn.few_queries_min_rows;
    const bool few_small = nq >= 2 && nq <= 3 && kn.filter_min_q == 2 && n > kFilterPhase0 && n < few_min;
    return ((int)nq >= kn.filter_min_q && !few_small) || single_filter || (nq == 1 && n <= kn.single_batched_max_rows);
}

// Step 2: the route, given whether index.hip obtained a filter copy (only ever when route_wants_filter said so).
inline SearchRoute plan_route(const RouteKnobs& kn, const SearchShape& s, bool have_copy) {
    SearchRoute r;
    // Two or more queries: the filter reads a quarter (int8) or half (f16) of the bytes of the f32 scan once for up to
    // 128 queries and the refine step keeps the result bit-identical.  One query stays on the streaming f32 scan
    // (the north-star kernel).  Without a filter copy, >= 5 queries use the exact-f32 MFMA path.
    if (have_copy) r.path = SearchPath::Filter;
    else if (s.normed && s.nq >= 5 && s.batched) r.path = SearchPath::BatchedExact;
    // A streaming scan of a few blocks (a corpus of the reference's own size: hundreds to thousands of chunks) reads
    // the queries straight from the pinned buffer too: a copy launch costs more than <= 64 blocks' reads over the link.
    if (!s.pinned) r.queries = QuerySource::Device;
    else if (r.path == SearchPath::Filter) r.queries = QuerySource::PrepPinned;
    else if (r.path == SearchPath::Stream && s.prime && s.stream_blocks <= 64) r.queries = QuerySource::StreamPinned;
    else r.queries = QuerySource::Copy;
    if (r.path == SearchPath::Stream) {
        const uint64_t rows = prime_rows_for(kn, s.n_rows, s.k, s.cus);
        const uint64_t min_rows = kn.prime_min_rows ? kn.prime_min_rows : (s.k >= 48 ? 100000 : 500000);
        if (kn.prime_min_k && s.k >= kn.prime_min_k && s.n_rows >= min_rows && s.n_rows >= 4 * rows && s.prime)
            r.prime_rows = rows;
    }
    return r;
}

}  // namespace cs
