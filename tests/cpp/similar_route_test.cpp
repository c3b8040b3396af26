// similar_route_test.cpp — the route of a similar-chunk search (codesearch_amd/csrc/similar_route.hpp) on the CPU: AUTO
// against the ordinary search's route (search_route.hpp) over a grid and at its thresholds, the preconditions, FILTER forced,
// SCAN forced.  Stand-alone: g++ -std=c++17 tests/cpp/similar_route_test.cpp && ./a.out
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../codesearch_amd/csrc/similar_route.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

static SearchShape shape(uint32_t nq, uint32_t k, uint64_t rows, uint32_t dim = 384) {
    SearchShape s;
    s.nq = nq; s.k = k; s.dim = dim; s.n_rows = rows;
    s.normed = true; s.use_split = true; s.batched = dim == 384 || dim == 768; s.prime = true; s.pinned = false;
    return s;
}

static SimilarRoute autoroute(const SearchShape& s, bool q8, bool copy = true, const RouteKnobs& kn = RouteKnobs()) {
    return plan_similar_route(kn, s, q8, copy, false, CS_SIMILAR_ROUTE_AUTO);
}

int main() {
    const SimilarRoute F = SimilarRoute::Filter, S = SimilarRoute::Scan;
    const uint64_t rows_grid[] = {1, 2, 1000, 1024, 1025, 3072, 3073, 16383, 16384, 20000, 32767, 32768, 39999, 40000,
                                  299999, 300000, 1999999, 2000000, 10000000};
    // AUTO = what an ordinary search of nq device-resident queries at this k does: the filter exactly when
    // route_wants_filter wants it, a copy was obtained and plan_route then answers Filter
    for (uint32_t nq : {1u, 2u, 3u, 4u, 5u, 9u, 40u, 130u})
        for (uint32_t k : {1u, 10u, 16u, 17u, 47u, 48u, 99u, 100u, 200u, 1000u})
            for (uint64_t rows : rows_grid)
                for (int q8 = 0; q8 < 2; ++q8)
                    for (int route : {CS_ROUTE_COST, CS_ROUTE_STREAM, CS_ROUTE_FILTER})
                        for (int copy = 0; copy < 2; ++copy) {
                            RouteKnobs kn;
                            kn.single_route = route;
                            const SearchShape s = shape(nq, k, rows);
                            const bool wants = route_wants_filter(kn, s, q8 != 0);
                            const bool filter = wants && copy && plan_route(kn, s, true).path == SearchPath::Filter;
                            CHECK(plan_similar_route(kn, s, q8 != 0, copy != 0, false, CS_SIMILAR_ROUTE_AUTO) == (filter ? F : S));
                            CHECK(similar_wants_filter(kn, s, q8 != 0, false, CS_SIMILAR_ROUTE_AUTO) == wants);
                            // SCAN forced: always the scan, and no copy is looked for
                            CHECK(plan_similar_route(kn, s, q8 != 0, copy != 0, false, CS_SIMILAR_ROUTE_SCAN) == S);
                            CHECK(!similar_wants_filter(kn, s, q8 != 0, false, CS_SIMILAR_ROUTE_SCAN));
                            // FILTER forced: sizes and the single-query route do not matter, the copy does
                            CHECK(plan_similar_route(kn, s, q8 != 0, copy != 0, false, CS_SIMILAR_ROUTE_FILTER) == (copy ? F : S));
                            // a scope: always the scan
                            for (int forced : {CS_SIMILAR_ROUTE_AUTO, CS_SIMILAR_ROUTE_SCAN, CS_SIMILAR_ROUTE_FILTER}) {
                                CHECK(plan_similar_route(kn, s, q8 != 0, copy != 0, true, forced) == S);
                                CHECK(!similar_wants_filter(kn, s, q8 != 0, true, forced));
                            }
                        }
    // the thresholds themselves, as numbers (search_route.hpp RouteKnobs' defaults)
    // ... the few-queries window: two or three sources between phase 0 and 16,384 rows (k <= 16) / 40,000 rows scan
    CHECK(autoroute(shape(2, 10, 3072), true) == F);
    CHECK(autoroute(shape(2, 10, 3073), true) == S);
    CHECK(autoroute(shape(2, 10, 16383), true) == S);
    CHECK(autoroute(shape(2, 10, 16384), true) == F);
    CHECK(autoroute(shape(3, 16, 16383), false) == S);
    CHECK(autoroute(shape(3, 17, 16384), true) == S);
    CHECK(autoroute(shape(3, 17, 39999), true) == S);
    CHECK(autoroute(shape(3, 17, 40000), true) == F);
    CHECK(autoroute(shape(4, 10, 5000), true) == F);
    CHECK(autoroute(shape(9, 200, 20000), true) == F);
    CHECK(autoroute(shape(130, 1, 3200), false) == F);
    // ... one source: the int8 copy's row counts by list length, the f16 copy's k and rows, the tiny-corpus batched window
    CHECK(autoroute(shape(1, 10, 32767), true) == S);
    CHECK(autoroute(shape(1, 10, 32768), true) == F);
    CHECK(autoroute(shape(1, 47, 32768), true) == F);
    CHECK(autoroute(shape(1, 48, 299999), true) == S);
    CHECK(autoroute(shape(1, 48, 300000), true) == F);
    CHECK(autoroute(shape(1, 10, 10000000), false) == S);
    CHECK(autoroute(shape(1, 99, 2000000), false) == S);
    CHECK(autoroute(shape(1, 100, 1999999), false) == S);
    CHECK(autoroute(shape(1, 100, 2000000), false) == F);
    CHECK(autoroute(shape(1, 10, 1024), false) == F);
    CHECK(autoroute(shape(1, 10, 1025), false) == S);
    {
        RouteKnobs stream;
        stream.single_route = CS_ROUTE_STREAM;  // cs_index_set_single_query_route(CS_ROUTE_STREAM): one source scans ...
        CHECK(autoroute(shape(1, 10, 10000000), true, true, stream) == S);
        CHECK(autoroute(shape(1, 200, 10000000), true, true, stream) == S);
        CHECK(autoroute(shape(9, 10, 10000000), true, true, stream) == F);  // ... nine do not
        CHECK(plan_similar_route(stream, shape(1, 10, 10000000), true, true, false, CS_SIMILAR_ROUTE_FILTER) == F);
        RouteKnobs never;
        never.filter_min_q = 1 << 20;  // cs_index_set_filter_min_queries: no multi-query filter
        CHECK(autoroute(shape(9, 10, 10000000), true, true, never) == S);
        CHECK(plan_similar_route(never, shape(9, 10, 10000000), true, true, false, CS_SIMILAR_ROUTE_FILTER) == F);
    }
    // the preconditions, under AUTO and under FILTER forced: a width the filter kernels lack, no filter copies kept, row
    // norms behind, no copy obtained — each one alone gives the scan
    for (int forced : {CS_SIMILAR_ROUTE_AUTO, CS_SIMILAR_ROUTE_FILTER}) {
        const RouteKnobs kn;
        CHECK(plan_similar_route(kn, shape(9, 10, 1000000), true, true, false, forced) == F);
        for (uint32_t dim : {100u, 128u, 512u, 1536u}) {
            CHECK(plan_similar_route(kn, shape(9, 10, 1000000, dim), true, true, false, forced) == S);
            CHECK(!similar_wants_filter(kn, shape(9, 10, 1000000, dim), true, false, forced));
        }
        for (uint32_t dim : {384u, 768u, 1024u}) CHECK(plan_similar_route(kn, shape(9, 10, 1000000, dim), true, true, false, forced) == F);
        SearchShape s = shape(9, 10, 1000000);
        s.use_split = false;
        CHECK(plan_similar_route(kn, s, false, true, false, forced) == S);
        CHECK(!similar_wants_filter(kn, s, false, false, forced));
        s = shape(9, 10, 1000000);
        s.normed = false;
        CHECK(plan_similar_route(kn, s, true, true, false, forced) == S);
        CHECK(!similar_wants_filter(kn, s, true, false, forced));
        CHECK(plan_similar_route(kn, shape(9, 10, 1000000), true, false, false, forced) == S);
    }
    // BatchedExact is never taken: five or more queries without a copy would go to the exact-f32 MFMA path as an ordinary
    // search; a similar call scans
    {
        const RouteKnobs kn;
        const SearchShape s = shape(9, 10, 1000000);
        CHECK(plan_route(kn, s, false).path == SearchPath::BatchedExact);
        CHECK(autoroute(s, true, false) == S);
        CHECK(plan_similar_route(kn, s, true, false, false, CS_SIMILAR_ROUTE_FILTER) == S);
    }
    // FILTER forced ignores sizes only: every shape of the few-queries window and under the one-source thresholds
    for (uint32_t nq : {1u, 2u, 3u})
        for (uint64_t rows : rows_grid) {
            const RouteKnobs kn;
            CHECK(plan_similar_route(kn, shape(nq, 10, rows), false, true, false, CS_SIMILAR_ROUTE_FILTER) == F);
            CHECK(similar_wants_filter(kn, shape(nq, 10, rows), false, false, CS_SIMILAR_ROUTE_FILTER));
        }
    if (failures) {
        std::printf("%d failure(s)\n", failures);
        return 1;
    }
    std::printf("similar route ok\n");
    return 0;
}
