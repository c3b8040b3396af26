// The grouped search over a sharded store on the CPU (codesearch_amd/csrc/shards_grouped_plan.hpp): the contract —
// capped_topk over the whole set under global ids — against what the device does: the rows dealt to shards by the stripe
// rule, capped_topk per shard over LOCAL ids (what a shard's capped scan and merge leave), the lists laid out as in the
// gather buffer, merged by the plan's levels: capped_shard_merge_block for the first, capped_merge_block for the rest.
// Key sets of 200 to 3,000 rows over 1 / 3 / 4 / 8 shards, stripes of 1 / 7 / 100 / more than the row count, k in
// {1, 10, 200, 1024}, per_group in {1, 3, k}; a group that fills every shard's list, cosine ties across shards, rows without
// a group, shards with fewer than k rows and with none; an uncapped first level that loses a row, an uncapped root that
// keeps too many; the id maps' round trip; the plan's level and scratch arithmetic.
//   shards_grouped_plan_test -> the checks below, "shards grouped plan ok"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/shards_grouped_plan.hpp"

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

struct Row { uint32_t cos_image, id, group; };

static bool same(const std::vector<GroupedRow>& a, const std::vector<GroupedRow>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].key != b[i].key || a[i].group != b[i].group) return false;
    return true;
}

static std::vector<GroupedRow> contract(const std::vector<Row>& rows, uint32_t k, uint32_t m) {
    std::vector<GroupedRow> all;
    for (const Row& r : rows) all.push_back(GroupedRow{key_of(r.cos_image, r.id), r.group});
    return capped_topk(all, k, m);
}

// Every shard's list for one query as it lies in the gather buffer: the capped best k of the shard's rows under LOCAL ids
// (m_shard = the cap the shards apply), k slots, zeros behind the count.
static std::vector<std::vector<uint64_t>> shard_lists(const std::vector<Row>& rows, uint32_t nshards, uint32_t stripe, uint32_t k,
                                                      uint32_t m_shard) {
    std::vector<std::vector<GroupedRow>> local(nshards);
    for (const Row& r : rows)
        local[shards_shard_of(r.id, stripe, nshards)].push_back(
            GroupedRow{key_of(r.cos_image, shards_local_of(r.id, stripe, nshards)), r.group});
    std::vector<std::vector<uint64_t>> lists(nshards);
    for (uint32_t s = 0; s < nshards; ++s) {
        for (const GroupedRow& r : capped_topk(local[s], k, m_shard)) lists[s].push_back(r.key);
        lists[s].resize(k, 0ull);
    }
    return lists;
}

// The launcher's sequence (launch_merge_shards_grouped): the shard merge in blocks of plan.group shards, then — when it
// left more than one list — launch_merge_grouped's loop over blocks of plan.rest.merge_group lists.  m_first / m_rest: the
// cap each level applies (the product: per_group everywhere).
static std::vector<GroupedRow> merge_by_plan(const std::vector<std::vector<uint64_t>>& lists, uint32_t stripe, uint32_t k,
                                             uint32_t m_first, uint32_t m_rest, const std::vector<uint32_t>& group_by_id,
                                             uint32_t* levels) {
    const uint32_t nshards = (uint32_t)lists.size();
    const ShardsGroupedPlan p = plan_shards_grouped(nshards, 1, k, false);
    auto group_of_id = [&](uint32_t id) { return id < group_by_id.size() ? group_by_id[id] : kNoGroup; };
    std::vector<std::vector<GroupedRow>> cur;
    for (uint32_t lo = 0; lo < nshards; lo += p.group) {
        const std::vector<std::vector<uint64_t>> part(lists.begin() + lo, lists.begin() + std::min(nshards, lo + p.group));
        cur.push_back(capped_shard_merge_block(part, lo, stripe, nshards, k, m_first, group_of_id));
    }
    CHECK(cur.size() == p.first_lists);
    *levels = 1;
    while (cur.size() > 1) {
        std::vector<std::vector<GroupedRow>> next;
        for (size_t lo = 0; lo < cur.size(); lo += p.rest.merge_group) {
            std::vector<GroupedRow> in;
            for (size_t l = lo; l < std::min(cur.size(), lo + p.rest.merge_group); ++l) in.insert(in.end(), cur[l].begin(), cur[l].end());
            CHECK(in.size() <= kGroupedMergeCap);
            next.push_back(capped_merge_block(in, k, m_rest));
        }
        cur = next;
        ++*levels;
    }
    CHECK(*levels == p.levels);
    return cur[0];
}

static std::vector<uint32_t> table_of(const std::vector<Row>& rows, uint32_t n_ids) {
    std::vector<uint32_t> t(n_ids, kNoGroup);
    for (const Row& r : rows) t[r.id] = r.group;
    return t;
}

static const uint32_t kShards[] = {1, 3, 4, 8};
static const uint32_t kKs[] = {1, 10, 200, 1024};

static void check_random_sets() {
    std::mt19937_64 rng(20241021);
    int trial = 0;
    for (uint32_t nshards : kShards)
        for (int si = 0; si < 4; ++si)
            for (uint32_t k : kKs)
                for (int mi = 0; mi < 3; ++mi, ++trial) {
                    const uint32_t n = 200 + (uint32_t)(rng() % 2801);
                    const uint32_t stripes[4] = {1, 7, 100, n + 1 + (uint32_t)(rng() % 50)};
                    const uint32_t stripe = stripes[si];
                    const uint32_t m = mi == 0 ? 1 : mi == 1 ? 3 : k;
                    const uint32_t ngroups = 1 + (uint32_t)(rng() % (trial % 4 == 0 ? 5 : 400));
                    const uint32_t distinct = trial % 3 == 0 ? 1 + (uint32_t)(rng() % 4) : 1 + (uint32_t)(rng() % 100000);  // few: ties
                    std::vector<Row> rows;
                    for (uint32_t id = 0; id < n; ++id) {
                        if (rng() % 10 == 0) continue;                       // a deleted id
                        uint32_t g = (uint32_t)(rng() % ngroups);
                        if (rng() % 10 < 3) g = kNoGroup;                    // 30 % without a group
                        if (trial % 5 == 0) g = id / 8 % ngroups;            // files of consecutive ids
                        rows.push_back(Row{(uint32_t)(rng() % distinct), id, g});
                    }
                    const std::vector<uint32_t> table = table_of(rows, n);
                    uint32_t levels = 0;
                    const std::vector<GroupedRow> got =
                        merge_by_plan(shard_lists(rows, nshards, stripe, k, m), stripe, k, m, m, table, &levels);
                    CHECK(same(got, contract(rows, k, m)));
                    if (failures) {
                        std::printf("  shards %u stripe %u n %u k %u m %u\n", nshards, stripe, n, k, m);
                        return;
                    }
                }
}

// One group holds the best rows of EVERY shard, at least k of them per shard: each shard's capped list carries per_group of
// it, the root meets nshards * per_group and has to cap again.  An uncapped root (m = k there) keeps them all.
static void check_spread_group() {
    for (uint32_t nshards : {3u, 4u, 8u})
        for (uint32_t stripe : {1u, 7u, 100u})
            for (uint32_t k : {10u, 200u})
                for (uint32_t m : {1u, 3u}) {
                    const uint32_t n = 3000;
                    std::vector<Row> rows;
                    for (uint32_t id = 0; id < n; ++id) {
                        const bool hog = id < nshards * stripe * ((k + stripe - 1) / stripe + 1);  // > k rows on every shard
                        rows.push_back(hog ? Row{1000000u + id % 17, id, 7u} : Row{id % 5000, id, 100u + id});
                    }
                    const std::vector<uint32_t> table = table_of(rows, n);
                    const auto lists = shard_lists(rows, nshards, stripe, k, m);
                    for (uint32_t s = 0; s < nshards; ++s) {  // the premise: every shard's list leads with m rows of the hog
                        uint32_t in_list = 0;
                        for (uint64_t key : lists[s]) in_list += key && table[shards_global_of(id_of(key), stripe, nshards, s)] == 7u;
                        CHECK(in_list == m);
                    }
                    uint32_t levels = 0;
                    const std::vector<GroupedRow> want = contract(rows, k, m);
                    CHECK(same(merge_by_plan(lists, stripe, k, m, m, table, &levels), want));
                    uint32_t hogs = 0;
                    for (const GroupedRow& r : want) hogs += r.group == 7u;
                    CHECK(hogs == m && want.size() == k);
                    const std::vector<GroupedRow> uncapped_root = merge_by_plan(lists, stripe, k, k, k, table, &levels);
                    hogs = 0;
                    for (const GroupedRow& r : uncapped_root) hogs += r.group == 7u;
                    CHECK(hogs == std::min(k, nshards * m) && !same(uncapped_root, want));
                }
}

// Equal cosines in different shards: the order is by global id, whatever the local ids are.
static void check_ties() {
    for (uint32_t nshards : {3u, 4u, 8u})
        for (uint32_t stripe : {1u, 7u, 100u}) {
            std::vector<Row> rows;
            for (uint32_t id = 0; id < 400; ++id) rows.push_back(Row{5u, id, id % 2 ? kNoGroup : id / 2 % 50});
            const std::vector<uint32_t> table = table_of(rows, 400);
            uint32_t levels = 0;
            const std::vector<GroupedRow> got = merge_by_plan(shard_lists(rows, nshards, stripe, 10, 1), stripe, 10, 1, 1, table, &levels);
            CHECK(same(got, contract(rows, 10, 1)));
            for (size_t i = 0; i < got.size(); ++i) CHECK(id_of(got[i].key) == (uint32_t)i);  // ids 0..9: 0, 2, ... open new groups
        }
}

// Shards with fewer than k rows, and with none: a stripe above the row count leaves everything on shard 0.
static void check_short_and_empty_shards() {
    std::vector<Row> rows;
    for (uint32_t id = 0; id < 200; ++id) rows.push_back(Row{id * 37 % 101, id, id / 8});
    const std::vector<uint32_t> table = table_of(rows, 200);
    for (uint32_t nshards : kShards)
        for (uint32_t stripe : {60u, 201u})
            for (uint32_t k : {10u, 1024u}) {
                const auto lists = shard_lists(rows, nshards, stripe, k, 3);
                if (stripe == 201u)
                    for (uint32_t s = 1; s < nshards; ++s) CHECK(lists[s][0] == 0ull);
                uint32_t levels = 0;
                CHECK(same(merge_by_plan(lists, stripe, k, 3, 3, table, &levels), contract(rows, k, 3)));
            }
}

// k = 2, per_group = 1, two shards, stripe 1.  Shard 0 holds a1, a2 (group 0) and b (group 1), best first; shard 1 holds c
// (group 2) below them all.  The contract keeps a1 and b.  A shard that does NOT cap sends {a1, a2}: b is in no list, and
// the root's answer is {a1, c}.
static void check_uncapped_first_level_loses_a_row() {
    const std::vector<Row> rows = {{90, 0, 0}, {80, 2, 0}, {70, 4, 1}, {10, 1, 2}};
    const std::vector<uint32_t> table = table_of(rows, 5);
    const std::vector<GroupedRow> want = contract(rows, 2, 1);
    CHECK(want.size() == 2 && id_of(want[0].key) == 0 && id_of(want[1].key) == 4);
    uint32_t levels = 0;
    CHECK(same(merge_by_plan(shard_lists(rows, 2, 1, 2, 1), 1, 2, 1, 1, table, &levels), want));
    const std::vector<GroupedRow> lost = merge_by_plan(shard_lists(rows, 2, 1, 2, /*m_shard=*/2), 1, 2, 1, 1, table, &levels);
    CHECK(lost.size() == 2 && id_of(lost[0].key) == 0 && id_of(lost[1].key) == 1);
}

static void check_id_maps() {
    for (uint32_t nshards : kShards)
        for (uint32_t stripe : {1u, 7u, 100u, (1u << 20) + 3u}) {
            std::vector<uint32_t> next_local(nshards, 0);  // a shard's local ids are dense and ascend with the global id
            for (uint32_t id = 0; id < (1u << 20); ++id) {
                const uint32_t s = shards_shard_of(id, stripe, nshards), l = shards_local_of(id, stripe, nshards);
                if (s >= nshards || l != next_local[s] || l > id || shards_global_of(l, stripe, nshards, s) != id) {
                    const bool round_trip = false;
                    CHECK(round_trip);
                    return;
                }
                ++next_local[s];
            }
        }
}

static void check_plan() {
    ShardsGroupedPlan p = plan_shards_grouped(4, 9, 1024, false);  // exactly kGroupedMergeCap keys: one level
    CHECK(p.group == 4 && p.first_lists == 1 && p.levels == 1 && p.scratch_keys == 0);
    p = plan_shards_grouped(8, 9, 1024, false);  // 8,192 keys at the root: two levels
    CHECK(p.group == 4 && p.first_lists == 2 && p.levels == 2 && p.first_keys == (size_t)9 * 2 * 1024 && p.merge_keys == 0);
    CHECK(p.rest.lists == 2 && p.rest.merge_group == 4 && p.scratch_keys == p.first_keys);
    p = plan_shards_grouped(64, 2, 1024, false);  // 64 -> 16 -> 4 -> 1
    CHECK(p.first_lists == 16 && p.levels == 3 && p.merge_keys == (size_t)2 * 4 * 1024);
    CHECK(p.scratch_keys == p.first_keys + 2 * p.merge_keys);
    p = plan_shards_grouped(4, 16, 1000, true);  // variants: the capped variants merge's two ping-pong buffers
    CHECK(p.first_lists == 1 && p.variants_keys == grouped_variants_tmp_keys(16, 1000) && p.scratch_keys == 2 * p.variants_keys);
    CHECK(plan_shards_grouped(1, 1, 1, false).levels == 1);
    for (uint32_t nshards = 1; nshards <= 64; ++nshards)
        for (uint32_t k = 1; k <= 1024; k += (k < 16 ? 1 : 61)) {
            p = plan_shards_grouped(nshards, 3, k, true);
            CHECK((uint64_t)p.group * k <= kGroupedMergeCap && p.group >= 2);
            CHECK(p.first_lists == (nshards + p.group - 1) / p.group && p.levels <= 3);
            CHECK((p.first_lists == 1) == (p.first_keys == 0));
        }
}

int main() {
    check_random_sets();
    check_spread_group();
    check_ties();
    check_short_and_empty_shards();
    check_uncapped_first_level_loses_a_row();
    check_id_maps();
    check_plan();
    if (failures) {
        std::printf("%d check(s) failed\n", failures);
        return 1;
    }
    std::printf("shards grouped plan ok\n");
    return 0;
}
