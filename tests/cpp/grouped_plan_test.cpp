// The host plan of a grouped search (codesearch_amd/csrc/grouped_plan.hpp) on the CPU: the scan geometry at 12 B per list
// slot, the merge levels, and the selection rule — the per-wave list step and the capped merge block, restated on the host
// as the kernels take them, against the contract (capped_topk) over random rows split into random parts.
//   grouped_plan_test -> the checks below, "grouped plan ok"
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/grouped_plan.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static void check_geometry() {
    const int cus = 256;
    for (uint32_t dim : {384u, 768u, 1024u, 100u, 4u}) {
        for (uint32_t k : {1u, 10u, 64u, 65u, 128u, 200u, 256u, 257u, 512u, 1000u, 1024u}) {
            for (uint32_t nq : {1u, 2u, 3u, 4u, 9u, 40u, 4096u}) {
                for (uint64_t n : {0ull, 1ull, 7ull, 1000ull, 12000ull, 1000000ull, 10000000ull}) {
                    const GroupedPlan p = plan_grouped(n, dim, nq, k, cus);
                    CHECK(p.kpad >= k && p.kpad >= 64 && (p.kpad & (p.kpad - 1)) == 0);
                    CHECK(p.qtile == 1 || p.qtile == 2 || p.qtile == 4);
                    CHECK(p.qtile <= nq);
                    CHECK(p.lds_bytes == (size_t)p.qtile * 4 * p.kpad * 12);
                    CHECK(p.lds_bytes <= kGroupedLdsBudget);
                    // the tile is the largest that fits
                    if (grouped_fast_dim(dim) && p.qtile < 4 && nq >= 2 * p.qtile)
                        CHECK((size_t)2 * p.qtile * 4 * p.kpad * 12 > kGroupedLdsBudget);
                    if (!grouped_fast_dim(dim)) CHECK(p.qtile == 1 && !p.deep);
                    CHECK(p.passes == (nq + p.qtile - 1) / p.qtile);
                    CHECK(p.blocks >= 1 && p.blocks <= (uint32_t)cus * 8);
                    CHECK(p.lists == p.blocks * 4);
                    CHECK(p.partial_keys == (size_t)nq * p.lists * k);
                    CHECK(p.partial_keys * 8 <= kGroupedPartialBudget || p.blocks == 1);
                    if (p.deep) CHECK(p.qtile == 1 && k <= 128 && p.blocks <= (uint32_t)cus);
                    // the merge: a block's keys fit, the levels reach one list, the scratch holds the first level
                    CHECK(p.merge_group >= 2 && (uint64_t)p.merge_group * k <= kGroupedMergeCap);
                    uint32_t lists = p.lists, levels = 0, first = 0;
                    do {
                        lists = (lists + p.merge_group - 1) / p.merge_group;
                        if (!levels) first = lists;
                        ++levels;
                    } while (lists > 1);
                    CHECK(levels == p.merge_levels);
                    CHECK(p.merge_keys == (first > 1 ? (size_t)nq * first * k : 0));
                }
            }
        }
    }
    // 12 B per slot lowers the tile where 8 B did not: kpad 1024 holds one query (48 KiB), kpad 512 two
    CHECK(plan_grouped(100000, 384, 9, 1024, cus).qtile == 1);
    CHECK(plan_grouped(100000, 384, 9, 512, cus).qtile == 2);
    CHECK(plan_grouped(100000, 384, 9, 256, cus).qtile == 4);
    // small stores launch few blocks; big ones one (deep) or two per CU
    CHECK(plan_grouped(1000, 384, 1, 10, cus).blocks == 16);  // 16 rows per deep tile, 4 waves
    CHECK(plan_grouped(10000000, 384, 1, 10, cus).blocks == 256);
    CHECK(plan_grouped(10000000, 384, 1, 200, cus).blocks == 512);
    CHECK(plan_grouped(10000000, 384, 1, 200, cus).merge_levels == 3);  // 2,048 lists of 200: 20 per block -> 103 -> 6 -> 1
}

static std::vector<GroupedRow> random_rows(std::mt19937_64& rng, size_t n, uint32_t ngroups, uint32_t distinct_cos) {
    std::vector<GroupedRow> rows(n);
    for (size_t i = 0; i < n; ++i) {
        // few distinct cosines: many ties, resolved by the id in the key's low half (~id: lower id = larger key)
        const uint64_t cosimg = 0x80000000u + (uint32_t)(rng() % distinct_cos);
        rows[i].key = (cosimg << 32) | (uint32_t)~(uint32_t)i;
        const uint32_t g = (uint32_t)(rng() % (ngroups + 1));
        rows[i].group = g == ngroups ? kNoGroup : g;
    }
    return rows;
}

static bool same(const std::vector<GroupedRow>& a, const std::vector<GroupedRow>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].key != b[i].key || a[i].group != b[i].group) return false;
    return true;
}

// rows (ascending id) dealt to `waves` lists as the scan deals tiles, each list stepped row by row; the lists merged in
// levels of `G` with the capped merge block; against the contract over all rows.
static void check_selection() {
    std::mt19937_64 rng(11);
    for (int rep = 0; rep < 400; ++rep) {
        const size_t n = 1 + rng() % 600;
        const uint32_t ngroups = 1 + (uint32_t)(rng() % 12);
        const uint32_t k = 1 + (uint32_t)(rng() % 40), m = 1 + (uint32_t)(rng() % 5);
        const uint32_t waves = 1 + (uint32_t)(rng() % 9), G = 2 + (uint32_t)(rng() % 3);
        const std::vector<GroupedRow> rows = random_rows(rng, n, ngroups, 1 + (uint32_t)(rng() % 50));
        const std::vector<GroupedRow> want = capped_topk(rows, k, m);
        std::vector<std::vector<GroupedRow>> lists(waves);
        for (size_t i = 0; i < n; ++i) capped_list_step(lists[(i / 8) % waves], rows[i], k, m);
        for (const auto& l : lists) {
            CHECK(l.size() <= k);
            // every wave's list is the capped top-k of the rows it met
            std::vector<GroupedRow> met;
            const size_t w = (size_t)(&l - lists.data());
            for (size_t i = 0; i < n; ++i)
                if ((i / 8) % waves == w) met.push_back(rows[i]);
            std::vector<GroupedRow> sorted = l;
            std::sort(sorted.begin(), sorted.end(), [](const GroupedRow& a, const GroupedRow& b) { return a.key > b.key; });
            CHECK(same(sorted, capped_topk(met, k, m)));
        }
        for (;;) {  // at least one level, as the search always launches one (it also sorts a single wave's list)
            std::vector<std::vector<GroupedRow>> next;
            for (size_t lo = 0; lo < lists.size(); lo += G) {
                std::vector<GroupedRow> all;
                for (size_t l = lo; l < lists.size() && l < lo + G; ++l) all.insert(all.end(), lists[l].begin(), lists[l].end());
                next.push_back(capped_merge_block(all, k, m));
            }
            lists.swap(next);
            if (lists.size() == 1) break;
        }
        CHECK(same(lists[0], want));
    }
    // an uncapped level loses rows the cap would promote, which is why every level caps: one group fills the plain top-3
    // of this part
    std::vector<GroupedRow> part;
    for (uint32_t i = 0; i < 6; ++i) part.push_back({((uint64_t)(0x80000100u - i) << 32) | (uint32_t)~i, i < 4 ? 0u : 1u + i});
    const std::vector<GroupedRow> capped = capped_merge_block(part, 3, 1);  // group 0 once, then groups 5 and 6
    CHECK(capped.size() == 3 && capped[0].group == 0 && capped[1].group == 5 && capped[2].group == 6);
    std::vector<GroupedRow> uncapped(part.begin(), part.begin() + 3);  // a plain top-3: all of group 0
    CHECK(capped_merge_block(uncapped, 3, 1).size() == 1);
    // per_group >= k, or no groups: the plain top-k
    for (int rep = 0; rep < 50; ++rep) {
        std::vector<GroupedRow> rows = random_rows(rng, 300, 3, 1000);
        std::vector<GroupedRow> plain = rows;
        std::sort(plain.begin(), plain.end(), [](const GroupedRow& a, const GroupedRow& b) { return a.key > b.key; });
        plain.resize(20);
        CHECK(same(capped_topk(rows, 20, 20), plain));
        CHECK(same(capped_merge_block(rows, 20, 0xFFFFFFFFu), plain));
        for (auto& r : rows) r.group = kNoGroup;
        for (auto& r : plain) r.group = kNoGroup;
        CHECK(same(capped_topk(rows, 20, 1), plain));
        CHECK(same(capped_merge_block(rows, 20, 1), plain));
    }
}

int main() {
    check_geometry();
    check_selection();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("grouped plan ok\n");
    return 0;
}
