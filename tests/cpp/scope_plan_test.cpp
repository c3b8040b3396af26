// The host plan of a search scope (codesearch_amd/csrc/masked_plan.hpp, "scopes") on the CPU: the ascending-ids check,
// the grid of the id-list pass, the refresh rule and the per-shard split of an id list against brute force.
//   scope_plan_test           -> the checks below, "scope plan ok"
//   scope_plan_test split S N -> reads ascending u32 ids (little-endian) from stdin until its end and writes, for each
//                                shard of a store of N shards in stripes of S, its id count (u64) and its local ids (u32)
//                                (tests/test_scope_host.py compares them with numpy)
//   scope_plan_test check     -> reads u32 ids from stdin and prints the first offending position, or -1
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/masked_plan.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void check_validation() {
    CHECK(scope_ids_first_unsorted(nullptr, 0) == -1);  // the empty scope, ids may be null
    const uint32_t one[] = {7};
    CHECK(scope_ids_first_unsorted(one, 1) == -1);
    const uint32_t asc[] = {0, 1, 5, 6, 0xFFFFFFFEu, 0xFFFFFFFFu};
    CHECK(scope_ids_first_unsorted(asc, 6) == -1);
    const uint32_t rep[] = {3, 4, 4, 9};  // a repeated id: the second of the pair
    CHECK(scope_ids_first_unsorted(rep, 4) == 2);
    const uint32_t uns[] = {3, 9, 8, 2};  // the FIRST offending position
    CHECK(scope_ids_first_unsorted(uns, 4) == 2);
    const uint32_t first[] = {1, 0};
    CHECK(scope_ids_first_unsorted(first, 2) == 1);
    const uint32_t last[] = {1, 2, 3, 3};
    CHECK(scope_ids_first_unsorted(last, 4) == 3);
    CHECK(scope_ids_first_unsorted(last, 3) == -1);  // ... and not past n
}

static void check_grid_and_refresh() {
    CHECK(scope_list_blocks(0) == 0 && scope_list_blocks(1) == 1 && scope_list_blocks(4095) == 1);
    CHECK(scope_list_blocks(4096) == 1 && scope_list_blocks(4097) == 2 && scope_list_blocks(8193) == 3);
    CHECK(scope_list_blocks(0xFFFFFFFFull) == (1u << 20));
    CHECK(scope_list_blocks(4096) == mask_list_blocks(4096));  // the same ids per block as the bitmap's row-list pass
    // a list is current exactly at the generation it was made at; generation 0 (never made) is always due
    CHECK(!scope_refresh_due(5, 5));
    CHECK(scope_refresh_due(5, 6) && scope_refresh_due(6, 5));
    CHECK(scope_refresh_due(0, 1));
}

// every id lands on the shard and at the local id the store gives it (shard_of / shard_local_id), in order
static void check_split() {
    std::mt19937_64 rng(23);
    const uint64_t stripes[] = {1, 7, 32, 100, 4096, 65536};
    for (uint64_t stripe : stripes)
        for (uint32_t n = 1; n <= 8; ++n)
            for (int rep = 0; rep < 3; ++rep) {
                const uint64_t next = 1 + rng() % 30000;  // ids issued: [0, next); the list reaches past them
                std::vector<uint32_t> ids;
                for (uint64_t g = 0; g < next + 500; ++g)
                    if (rng() % 4 == 0) ids.push_back((uint32_t)g);
                CHECK(scope_ids_first_unsorted(ids.data(), ids.size()) == -1);
                std::vector<std::vector<uint32_t>> out;
                shard_scope_ids(ids.data(), ids.size(), stripe, n, out);
                CHECK(out.size() == n);
                // local ids a shard has issued: those of the global ids below next it holds
                std::vector<uint64_t> issued(n, 0);
                for (uint64_t g = 0; g < next; ++g) issued[shard_of(g, stripe, n)] += 1;
                std::vector<size_t> at(n, 0);
                size_t total = 0;
                for (uint32_t g : ids) {
                    const uint32_t s = shard_of(g, stripe, n);
                    CHECK(at[s] < out[s].size());
                    if (at[s] >= out[s].size()) return;
                    const uint32_t l = out[s][at[s]++];
                    CHECK(l == shard_local_id(g, stripe, n));
                    // a list that straddles the issued ids: issued global ids are issued local ids, the others are not
                    CHECK((g < next) == (l < issued[s]));
                }
                for (uint32_t s = 0; s < n; ++s) {
                    CHECK(at[s] == out[s].size());
                    CHECK(scope_ids_first_unsorted(out[s].data(), out[s].size()) == -1);  // still strictly ascending
                    total += out[s].size();
                }
                CHECK(total == ids.size());
            }
    std::vector<std::vector<uint32_t>> out;
    shard_scope_ids(nullptr, 0, 100, 3, out);  // the empty scope: one empty list per shard
    CHECK(out.size() == 3 && out[0].empty() && out[1].empty() && out[2].empty());
    const uint32_t top[] = {0xFFFFFFFFu};  // the largest id keeps a local id that fits u32
    shard_scope_ids(top, 1, 1, 1, out);
    CHECK(out[0].size() == 1 && out[0][0] == 0xFFFFFFFFu);
}

static std::vector<uint32_t> read_ids() {
    std::vector<uint32_t> ids;
    uint32_t buf[4096];
    size_t got;
    while ((got = std::fread(buf, sizeof(uint32_t), 4096, stdin)) > 0) ids.insert(ids.end(), buf, buf + got);
    return ids;
}

int main(int argc, char** argv) {
    if (argc == 4 && std::strcmp(argv[1], "split") == 0) {
        const uint64_t stripe = std::strtoull(argv[2], nullptr, 10);
        const uint32_t n = (uint32_t)std::strtoul(argv[3], nullptr, 10);
        const std::vector<uint32_t> ids = read_ids();
        std::vector<std::vector<uint32_t>> out;
        shard_scope_ids(ids.data(), ids.size(), stripe, n, out);
        for (uint32_t s = 0; s < n; ++s) {
            const uint64_t cnt = out[s].size();
            std::fwrite(&cnt, sizeof cnt, 1, stdout);
            if (cnt) std::fwrite(out[s].data(), sizeof(uint32_t), out[s].size(), stdout);
        }
        return 0;
    }
    if (argc == 2 && std::strcmp(argv[1], "check") == 0) {
        const std::vector<uint32_t> ids = read_ids();
        std::printf("%lld\n", (long long)scope_ids_first_unsorted(ids.data(), ids.size()));
        return 0;
    }
    if (argc > 1) return 2;
    check_validation();
    check_grid_and_refresh();
    check_split();
    if (failures) return 1;
    std::printf("scope plan ok\n");
    return 0;
}
