// shards_grouped_plan.hpp — the host side of a grouped search over a sharded store (shards.hip cs_shards_search_grouped*,
// scan_shards_grouped.hip): the exact best k rows of the whole store such that no group contributes more than per_group of
// them.  Plain C++17, no HIP: tests/cpp/shards_grouped_plan_test.cpp checks it on the CPU, and shards.hip only launches
// what it returns.
//
// No new lemma: a shard is a part.  grouped_plan.hpp shows that a row in the capped top-k of a union is in the capped
// top-k of its own part, so the capped top-k of the concatenated capped lists is the answer PROVIDED EVERY level caps.
// Every shard's grouped device search leaves its capped best k (capped scan + capped merge under the shard's own table,
// local ids); the root caps again while it merges, under a table by GLOBAL id.  A group whose rows are spread over the
// shards fills per_group slots of every shard's list, so the root's cap is not optional: an uncapped root merge keeps up
// to nshards * per_group rows of it and drops rows of other groups that the contract keeps (the CPU test shows one).
//
// Ids: the stripe rule of shards.hip.  Stripe t = id / stripe lives on shard t % N as local stripe t / N; the functions
// below are that rule in both directions, for the host (cs_shards_set_groups restates global ids as (shard, local id))
// and for the root's merge kernel (local row -> global id while it reads the lists).  The map is monotone inside a shard,
// so a shard's order under (cosine desc, local id asc) is its order under (cosine desc, global id asc).
//
// Levels: the gather buffer holds list s of query q at (s * nq + q) * k.  A block of the shard merge takes one query and
// up to G = kGroupedMergeCap / k shards.  N <= G: one level, the result is final.  Otherwise the first level writes
// [nq][ceil(N / G)][k] capped lists of GLOBAL keys and the ordinary capped merge (launch_merge_grouped) finishes under the
// root's table; N <= 64 and G >= 4 make that at most two more levels.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "grouped_plan.hpp"

#if defined(__HIPCC__)
#define CS_SHARDS_HD __host__ __device__ __forceinline__
#else
#define CS_SHARDS_HD inline
#endif

namespace cs {

// ---- (shard, local id) <-> global id ---------------------------------------------------------------------
CS_SHARDS_HD uint32_t shards_shard_of(uint32_t id, uint32_t stripe, uint32_t nshards) { return (id / stripe) % nshards; }
CS_SHARDS_HD uint32_t shards_local_of(uint32_t id, uint32_t stripe, uint32_t nshards) {
    return ((id / stripe) / nshards) * stripe + id % stripe;  // never above id
}
// (shard, local) of an id the store has issued -> that id; for such pairs the product stays below 2^32
CS_SHARDS_HD uint32_t shards_global_of(uint32_t local, uint32_t stripe, uint32_t nshards, uint32_t shard) {
    return ((local / stripe) * nshards + shard) * stripe + local % stripe;
}

// ---- levels and scratch -----------------------------------------------------------------------------------
struct ShardsGroupedPlan {
    uint32_t group = 2;        // shards a block of the shard merge takes (G)
    uint32_t first_lists = 1;  // lists per query the shard merge leaves: ceil(N / G); 1: its result is final
    uint32_t levels = 1;       // the shard merge + the capped merges behind it
    size_t first_keys = 0;     // nq * first_lists * k when first_lists > 1: the shard merge's output
    size_t merge_keys = 0;     // one ping-pong buffer of the capped merges behind it (0: they are one level)
    size_t variants_keys = 0;  // one ping-pong buffer of the capped variants merge (variants searches only)
    // keys of root scratch behind the shard slots and the spare [nq][k] block: first level, two ping-pong buffers of the
    // list merge, two of the variants merge
    size_t scratch_keys = 0;
    GroupedPlan rest;          // what launch_merge_grouped reads when first_lists > 1: lists, merge_group
};

inline ShardsGroupedPlan plan_shards_grouped(uint32_t nshards, uint32_t nq, uint32_t k, bool variants) {
    ShardsGroupedPlan p;
    p.group = grouped_merge_group(k);
    p.first_lists = (nshards + p.group - 1) / p.group;
    if (p.first_lists < 1) p.first_lists = 1;
    if (p.first_lists > 1) {
        p.first_keys = (size_t)nq * p.first_lists * k;
        p.rest.lists = p.first_lists;
        p.rest.merge_group = p.group;
        p.rest.merge_levels = grouped_merge_levels(p.first_lists, k);
        const uint32_t second = (p.first_lists + p.group - 1) / p.group;
        p.rest.merge_keys = second > 1 ? (size_t)nq * second * k : 0;
        p.merge_keys = p.rest.merge_keys;
        p.levels = 1 + p.rest.merge_levels;
    }
    p.variants_keys = variants ? grouped_variants_tmp_keys(nq, k) : 0;
    p.scratch_keys = p.first_keys + 2 * p.merge_keys + 2 * p.variants_keys;
    return p;
}

// ---- one block of the shard merge on the host ------------------------------------------------------------
// lists[i] = the capped best k of shard first_shard + i for one query as it lies in the gather buffer: keys carry LOCAL
// rows, empty slots are 0 (their group is not read).  `group_of_id` = the root's table: global id -> group.  The block
// restates every key under its global id, looks its group up, and is capped_topk from there (the kernel's sort, image
// sort, cut and compaction are capped_merge_block's, which tests/cpp/grouped_plan_test.cpp holds against capped_topk).
template <class GroupOf>
inline std::vector<GroupedRow> capped_shard_merge_block(const std::vector<std::vector<uint64_t>>& lists, uint32_t first_shard,
                                                        uint32_t stripe, uint32_t nshards, uint32_t k, uint32_t m,
                                                        GroupOf&& group_of_id) {
    std::vector<GroupedRow> rows;
    for (size_t i = 0; i < lists.size(); ++i)
        for (const uint64_t key : lists[i]) {
            if (!key) continue;
            const uint32_t gid = shards_global_of(~(uint32_t)key, stripe, nshards, first_shard + (uint32_t)i);
            rows.push_back(GroupedRow{(key & 0xffffffff00000000ull) | (uint64_t)(uint32_t)~gid, group_of_id(gid)});
        }
    return capped_topk(rows, k, m);
}

}  // namespace cs
