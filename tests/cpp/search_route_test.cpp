// The route of an index search (codesearch_amd/csrc/search_route.hpp) on the CPU: whether it wants the filter, which path
// answers it, where its queries are read from and the prime pass.  Every expected route below was recorded from the
// decision expressions of index.hip run_search as they stood before the route was split out of it (cus = 256).  Form of a
// route: "<want | -> <stream | filter | exact> <device | prep | pinned | copy>[ prime <sample rows>]": "want" = the search
// looks for a filter copy; the queries come from the caller's device buffer, the filter's prep kernel reading the pinned
// buffer, the streaming scan reading it directly, or one H2D copy.
#include <cstdio>
#include <string>

#include "../../codesearch_amd/csrc/search_route.hpp"

using namespace cs;

enum Knobs { kDefault, kMinQ1, kMinQ3, kStream, kFilter, kMinK0, kBatched0, kPrime0, kNoSplit };

struct RouteCase {
    Knobs knobs;
    uint32_t dim;
    uint64_t rows;
    uint32_t nq, k;
    int q8_serves;      // the int8 copy serves
    int copy;           // a filter copy is obtained when the search wants one
    int pinned;         // host-buffer API: the queries are in pinned memory
    uint64_t blocks;    // the streaming plan's blocks x passes
    const char* route;
};

static const RouteCase kCases[] = {
    // one query: the int8 crossovers, both sides of 32,768 and 300,000 rows at k = 47 and 48
    {kDefault, 384, 32767, 1, 47, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 32768, 1, 47, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 32768, 1, 48, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 299999, 1, 47, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 299999, 1, 48, 1, 1, 1, 2048, "- stream copy prime 4096"},
    {kDefault, 384, 300000, 1, 48, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 300000, 1, 48, 0, 1, 1, 2048, "- stream copy prime 4096"},
    // two to four queries: both sides of 16,384 and 40,000 rows at k = 16 and 17
    {kDefault, 384, 16383, 2, 16, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 16384, 2, 16, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 16384, 2, 17, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 39999, 2, 17, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 40000, 2, 17, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 16383, 3, 16, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 16384, 3, 16, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 39999, 3, 17, 1, 1, 1, 2048, "- stream copy"},
    {kDefault, 384, 40000, 3, 17, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 16383, 4, 16, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 39999, 4, 17, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 40000, 4, 17, 1, 1, 1, 2048, "want filter prep"},
    // phase 0: at or below 3,072 rows two queries take the filter
    {kDefault, 384, 3072, 2, 10, 0, 1, 1, 16, "want filter prep"},
    {kDefault, 384, 3073, 2, 10, 0, 1, 1, 16, "- stream pinned"},
    // one query over a corpus of the reference's own size: the batched path up to 1,024 rows
    {kDefault, 384, 1024, 1, 10, 0, 1, 1, 16, "want filter prep"},
    {kDefault, 384, 1025, 1, 10, 0, 1, 1, 16, "- stream pinned"},
    {kBatched0, 384, 1024, 1, 10, 0, 1, 1, 16, "- stream pinned"},
    // one query with only the f16 copy: from k = 100 over >= 2M rows
    {kDefault, 384, 1999999, 1, 100, 0, 1, 1, 2048, "- stream copy prime 7808"},
    {kDefault, 384, 2000000, 1, 99, 0, 1, 1, 2048, "- stream copy prime 7808"},
    {kDefault, 384, 2000000, 1, 100, 0, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 2000000, 1, 100, 0, 0, 1, 2048, "want stream copy prime 7808"},
    // five queries and more: the filter with a copy, the exact-f32 MFMA path without (none at 1024), both APIs
    {kDefault, 384, 50000, 9, 10, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 50000, 9, 10, 1, 0, 1, 2048, "want exact copy"},
    {kDefault, 768, 50000, 9, 10, 1, 1, 0, 2048, "want filter device"},
    {kDefault, 768, 50000, 9, 10, 1, 0, 0, 2048, "want exact device"},
    {kDefault, 1024, 50000, 9, 10, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 1024, 50000, 9, 10, 1, 0, 1, 2048, "want stream copy"},
    {kDefault, 1024, 50000, 5, 200, 1, 0, 0, 2048, "want stream device"},
    {kNoSplit, 384, 50000, 5, 10, 0, 0, 1, 2048, "- exact copy"},
    // CS_FILTER_MIN_Q
    {kMinQ1, 384, 100000, 1, 10, 0, 1, 1, 2048, "want filter prep"},
    {kMinQ1, 384, 10000, 2, 10, 0, 1, 1, 2048, "want filter prep"},
    {kMinQ3, 384, 1000000, 2, 10, 1, 1, 1, 2048, "- stream copy prime 4096"},
    {kMinQ3, 384, 10000, 3, 10, 1, 1, 1, 2048, "want filter prep"},
    // single-query routes
    {kStream, 384, 10000000, 1, 10, 1, 1, 1, 2048, "- stream copy prime 8192"},
    {kStream, 384, 1000, 1, 10, 1, 1, 1, 16, "want filter prep"},
    {kStream, 384, 10000, 2, 10, 1, 1, 1, 2048, "- stream copy"},
    {kFilter, 384, 5000, 1, 10, 0, 1, 1, 2048, "want filter prep"},
    {kFilter, 384, 5000, 1, 10, 0, 0, 1, 2048, "want stream copy"},
    {kMinK0, 384, 10000000, 1, 200, 1, 1, 1, 2048, "- stream copy prime 16384"},
    {kMinK0, 384, 1000, 1, 10, 1, 1, 1, 16, "want filter prep"},
    // prime rows over 1M and 10M rows
    {kDefault, 384, 1000000, 1, 10, 0, 0, 0, 2048, "- stream device prime 4096"},
    {kDefault, 384, 1000000, 1, 16, 0, 0, 0, 2048, "- stream device prime 4096"},
    {kDefault, 384, 1000000, 1, 17, 0, 0, 0, 2048, "- stream device prime 4096"},
    {kDefault, 384, 1000000, 1, 200, 0, 0, 0, 2048, "- stream device prime 4096"},
    {kDefault, 384, 1000000, 1, 300, 0, 0, 0, 2048, "- stream device prime 65536"},
    {kDefault, 384, 1000000, 1, 1024, 0, 0, 0, 2048, "- stream device prime 131072"},
    {kDefault, 384, 10000000, 1, 10, 0, 0, 0, 2048, "- stream device prime 8192"},
    {kDefault, 384, 10000000, 1, 16, 0, 0, 0, 2048, "- stream device prime 8192"},
    {kDefault, 384, 10000000, 1, 17, 0, 0, 0, 2048, "- stream device prime 16384"},
    {kDefault, 384, 10000000, 1, 200, 0, 0, 0, 2048, "want stream device prime 16384"},
    {kDefault, 384, 10000000, 1, 300, 0, 0, 0, 2048, "want stream device prime 65536"},
    {kDefault, 384, 10000000, 1, 1024, 0, 0, 0, 2048, "want stream device prime 131072"},
    {kStream, 768, 1000000, 2, 200, 1, 1, 1, 2048, "want filter prep"},
    {kDefault, 384, 499999, 1, 47, 0, 0, 0, 2048, "- stream device"},
    {kDefault, 384, 500000, 1, 47, 0, 0, 0, 2048, "- stream device prime 4096"},
    {kDefault, 384, 99999, 1, 48, 0, 0, 0, 2048, "- stream device"},
    {kDefault, 384, 100000, 1, 48, 0, 0, 0, 2048, "- stream device prime 4096"},
    // no prime pass: CS_SCAN_PRIME_MIN_K=0, and a dim without it
    {kPrime0, 384, 10000000, 1, 200, 0, 0, 0, 2048, "want stream device"},
    {kDefault, 512, 10000000, 1, 200, 0, 0, 0, 2048, "- stream device"},
    {kDefault, 512, 10000000, 1, 200, 0, 0, 1, 2048, "- stream copy"},
    // the streaming scan reads pinned queries directly up to 64 blocks x passes
    {kDefault, 384, 1500, 1, 10, 0, 1, 1, 64, "- stream pinned"},
    {kDefault, 384, 1500, 1, 10, 0, 1, 1, 65, "- stream copy"},
    {kDefault, 384, 1500, 1, 10, 0, 1, 0, 64, "- stream device"},
    {kDefault, 512, 1500, 1, 10, 0, 0, 1, 64, "- stream copy"},
    {kDefault, 384, 10000, 2, 10, 1, 1, 1, 64, "- stream pinned"},
    {kDefault, 384, 10000, 2, 10, 1, 1, 1, 65, "- stream copy"},
};

static std::string route_of(const RouteCase& c) {
    RouteKnobs kn;
    if (c.knobs == kMinQ1) kn.filter_min_q = 1;                 // CS_FILTER_MIN_Q=1
    if (c.knobs == kMinQ3) kn.filter_min_q = 3;                 // CS_FILTER_MIN_Q=3
    if (c.knobs == kStream) kn.single_route = CS_ROUTE_STREAM;  // cs_index_set_single_query_route
    if (c.knobs == kFilter) kn.single_route = CS_ROUTE_FILTER;
    if (c.knobs == kMinK0) {                                    // CS_FILTER_SINGLE_MIN_K=0
        kn.single_filter_min_k = 0;
        kn.single_route = CS_ROUTE_STREAM;
    }
    if (c.knobs == kBatched0) kn.single_batched_max_rows = 0;   // CS_SINGLE_BATCHED_MAX_ROWS=0
    if (c.knobs == kPrime0) kn.prime_min_k = 0;                 // CS_SCAN_PRIME_MIN_K=0
    const bool fast = c.dim == 384 || c.dim == 768 || c.dim == 1024;
    SearchShape s;
    s.nq = c.nq;
    s.k = c.k;
    s.dim = c.dim;
    s.n_rows = c.rows;
    s.cus = 256;
    s.normed = true;
    s.use_split = fast && c.knobs != kNoSplit;  // split_scan_supported; kNoSplit: CS_INDEX_SPLIT=0
    s.batched = c.dim == 384 || c.dim == 768;   // batched_supported
    s.prime = fast;                             // scan_prime_supported
    s.pinned = c.pinned;
    s.stream_blocks = c.blocks;
    const bool want = route_wants_filter(kn, s, c.q8_serves);
    const SearchRoute r = plan_route(kn, s, want && c.copy);
    static const char* path[] = {"stream", "filter", "exact"};
    static const char* src[] = {"device", "prep", "pinned", "copy"};
    std::string out = std::string(want ? "want " : "- ") + path[(int)r.path] + " " + src[(int)r.queries];
    if (r.prime_rows) out += " prime " + std::to_string(r.prime_rows);
    return out;
}

int main() {
    int bad = 0, n = 0;
    for (const RouteCase& c : kCases) {
        ++n;
        const std::string got = route_of(c);
        if (got != c.route) {
            printf("case %d (dim %u, %llu rows, nq %u, k %u): expected \"%s\", got \"%s\"\n", n, c.dim, (unsigned long long)c.rows,
                   c.nq, c.k, c.route, got.c_str());
            ++bad;
        }
    }
    if (bad) return 1;
    printf("search route ok: %d cases\n", n);
    return 0;
}
