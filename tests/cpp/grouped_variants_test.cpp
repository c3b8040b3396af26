// The grouped variants search on the CPU (codesearch_amd/csrc/grouped_plan.hpp): the contract — a row's key is the best of
// its keys over the query variants, then the capped walk — against what the device does: one capped list per variant
// (capped_topk: what the capped scan and merge leave for one query), merged by capped_variants_merge_block, the host
// statement of merge_variants_grouped_kernel, in one level and in levels of 2 to 4 variants per block.  Small universes
// (at most 40 ids, 6 groups and CS_NO_GROUP, k <= 8, per_group <= 3, 1 to 9 variants), cosine ties and identical variants
// included; a concrete case in which uncapped per-variant lists lose a row; the merge's level arithmetic.
//   grouped_variants_test -> the checks below, "grouped variants ok"
#include <algorithm>
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

// a packed key as the kernels build it: an order-preserving cosine image above ~id (lower id = larger key)
static uint64_t key_of(uint32_t cos_image, uint32_t id) { return ((uint64_t)(0x80000000u + cos_image) << 32) | (uint32_t)~id; }
static uint32_t id_of(uint64_t key) { return ~(uint32_t)key; }

static bool same(const std::vector<GroupedRow>& a, const std::vector<GroupedRow>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].key != b[i].key || a[i].group != b[i].group) return false;
    return true;
}

// The contract: every id's best key over the variants, then the capped walk.
static std::vector<GroupedRow> contract(const std::vector<std::vector<GroupedRow>>& variants, uint32_t k, uint32_t m) {
    std::vector<GroupedRow> best;
    for (const auto& v : variants)
        for (const GroupedRow& r : v) {
            auto it = std::find_if(best.begin(), best.end(), [&](const GroupedRow& o) { return id_of(o.key) == id_of(r.key); });
            if (it == best.end()) best.push_back(r);
            else if (r.key > it->key) *it = r;
        }
    return capped_topk(best, k, m);
}

// A list as it lies in HBM: k slots, the empty ones 0.
static void append_list(std::vector<GroupedRow>& out, const std::vector<GroupedRow>& list, uint32_t k) {
    out.insert(out.end(), list.begin(), list.end());
    for (size_t i = list.size(); i < k; ++i) out.push_back(GroupedRow{0ull, 0u});
}

// The launcher's loop (launch_merge_variants_grouped): blocks of G lists until one list is left.
static std::vector<GroupedRow> merge_in_levels(std::vector<std::vector<GroupedRow>> lists, uint32_t k, uint32_t m, uint32_t G,
                                               uint32_t* levels) {
    *levels = 0;
    for (;;) {
        std::vector<std::vector<GroupedRow>> next;
        for (size_t lo = 0; lo < lists.size(); lo += G) {
            std::vector<GroupedRow> in;
            for (size_t l = lo; l < std::min(lists.size(), lo + G); ++l) append_list(in, lists[l], k);
            next.push_back(capped_variants_merge_block(in, k, m));
        }
        ++*levels;
        if (next.size() == 1) return next[0];
        lists = next;
    }
}

static void check_universes() {
    std::mt19937_64 rng(20240611);
    for (int trial = 0; trial < 6000; ++trial) {
        const uint32_t n = 1 + (uint32_t)(rng() % 40), ngroups = 1 + (uint32_t)(rng() % 6);
        const uint32_t k = 1 + (uint32_t)(rng() % 8), m = 1 + (uint32_t)(rng() % 3), nv = 1 + (uint32_t)(rng() % 9);
        const uint32_t distinct = 1 + (uint32_t)(rng() % (trial % 3 == 0 ? 3 : 30));  // few cosines: many ties
        std::vector<uint32_t> group(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t g = (uint32_t)(rng() % (ngroups + 1));
            group[i] = g == ngroups ? kNoGroup : g;
        }
        std::vector<std::vector<GroupedRow>> variants(nv);
        for (uint32_t v = 0; v < nv; ++v) {
            if (v > 0 && rng() % 4 == 0) {  // an exact copy of an earlier variant
                variants[v] = variants[rng() % v];
                continue;
            }
            for (uint32_t i = 0; i < n; ++i) variants[v].push_back(GroupedRow{key_of((uint32_t)(rng() % distinct), i), group[i]});
        }
        const std::vector<GroupedRow> want = contract(variants, k, m);
        std::vector<std::vector<GroupedRow>> lists;
        for (const auto& v : variants) lists.push_back(capped_topk(v, k, m));
        uint32_t levels = 0;
        const std::vector<GroupedRow> one = merge_in_levels(lists, k, m, 9, &levels);
        CHECK(levels == 1);
        CHECK(same(one, want));
        for (uint32_t G = 2; G <= 4; ++G) {
            const std::vector<GroupedRow> got = merge_in_levels(lists, k, m, G, &levels);
            CHECK(same(got, want));
            uint32_t expect = 1, l = nv;
            while ((l = (l + G - 1) / G) > 1) ++expect;
            CHECK(levels == expect);
        }
        // per_group >= k: the plain variants merge (best key per id, best k)
        const std::vector<GroupedRow> plain = contract(variants, k, k);
        std::vector<GroupedRow> all;
        for (const auto& v : variants) all.insert(all.end(), v.begin(), v.end());
        CHECK(same(capped_variants_merge_block(all, k, k), plain));
        if (failures) return;
    }
}

// k = 2, per_group = 1, two identical variants: a1 and a2 (group 0) lead, b (group 1) is third.  The contract keeps a1 and
// b.  The UNCAPPED top-2 of either variant is {a1, a2}: de-duplicated and capped, the union holds a1 alone and b is lost.
static void check_counterexample() {
    const std::vector<GroupedRow> v = {{key_of(90, 0), 0u}, {key_of(80, 1), 0u}, {key_of(70, 2), 1u}, {key_of(60, 3), 2u}};
    const std::vector<std::vector<GroupedRow>> variants = {v, v};
    const std::vector<GroupedRow> want = contract(variants, 2, 1);
    CHECK(want.size() == 2 && id_of(want[0].key) == 0 && id_of(want[1].key) == 2);
    std::vector<GroupedRow> capped, uncapped;
    for (const auto& x : variants) {
        append_list(capped, capped_topk(x, 2, 1), 2);
        append_list(uncapped, capped_topk(x, 2, 2), 2);  // per_group = k: the plain top-2
    }
    CHECK(same(capped_variants_merge_block(capped, 2, 1), want));
    const std::vector<GroupedRow> lost = capped_variants_merge_block(uncapped, 2, 1);
    CHECK(lost.size() == 1 && id_of(lost[0].key) == 0);
}

static void check_levels() {
    CHECK(grouped_variants_levels(9, 1024) == 2 && grouped_variants_tmp_keys(9, 1024) == (size_t)3 * 1024);
    CHECK(grouped_variants_levels(16, 1024) == 2 && grouped_variants_tmp_keys(16, 1024) == (size_t)4 * 1024);
    CHECK(grouped_variants_levels(9, 455) == 1 && grouped_variants_tmp_keys(9, 455) == 0);
    CHECK(grouped_variants_levels(9, 456) == 2 && grouped_variants_tmp_keys(9, 456) == (size_t)2 * 456);
    CHECK(grouped_variants_levels(1, 1024) == 1 && grouped_variants_tmp_keys(1, 1024) == 0);
    for (uint32_t k = 1; k <= 1024; ++k)
        for (uint32_t nv = 1; nv <= 16; ++nv) {
            const uint32_t G = grouped_merge_group(k);
            CHECK(G >= 2 && (uint64_t)G * k <= kGroupedMergeCap);
            CHECK(grouped_variants_levels(nv, k) <= 2);  // one ping-pong buffer is ever written
            CHECK(grouped_variants_tmp_keys(nv, k) <= (size_t)kGroupedMergeCap * 2);
        }
}

int main() {
    check_universes();
    check_counterexample();
    check_levels();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("grouped variants ok\n");
    return 0;
}
