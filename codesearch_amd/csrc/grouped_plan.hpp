// grouped_plan.hpp — the host side of a grouped search (scan_grouped.hip): the exact best k rows such that no group
// (a chunk's file) contributes more than per_group of them.  Plain C++17, no HIP: tests/cpp/grouped_plan_test.cpp checks
// it on the CPU, and index.hip only launches what it returns.
//
// The contract (include/codesearch_gpu.h, cs_index_search_grouped): order the live rows by (cosine desc, id asc), walk
// that order, keep a row when its group is CS_NO_GROUP or fewer than per_group rows of its group have been kept, stop at
// k kept rows.  capped_topk below is that sentence as code; the CPU test compares the kernels' selection rule with it.
//
// Why partial lists can be merged: a row that is in the capped top-k of a union is in the capped top-k of its own part —
// for every group h, min(m, rows of h in the part that beat it) <= min(m, rows of h anywhere that beat it), so the row
// is kept no later in the part than in the union.  The capped top-k of the concatenated capped lists is therefore the
// answer, PROVIDED EVERY level caps: an uncapped level can drop a row that the cap would have promoted.  The scan's
// per-wave lists are capped lists, the scan does not merge them (that would be a level), and every level of the key merge
// caps, so a search is: one scan launch that leaves kScanWaves lists per block, then merge_levels capped merges.
//
// No prime pass: the k-th largest wave maximum bounds the k-th best cosine from below only because the maxima belong to
// k different rows; under a cap those rows may share a group and the capped k-th can lie below it.
//
// A scope (cs_index_search_grouped_scoped) changes the rows in play, not the rule: the scan walks the scope's row list
// (live rows only, ascending) and plan_grouped is called with the list's length where the stored rows go.  The list needs
// no other answer from the plan: the same LDS and partial-list budgets, the same merge levels.
//
// Query variants under the cap (cs_index_search_variants_grouped): a row's key is s(c) = the best of its keys over the
// set V of variants, and the answer is the capped top-k under s.  Why per-variant capped lists can be merged: let s(c) be
// reached in variant v, and let c be missing from v's capped top-k.  Then, in v's order, either per_group rows of c's
// group beat c — under s each of them keeps a key at least as large, and s(c) is c's key in v, so they beat c under s —
// or k cap-valid rows beat c in v: their s-keys beat c too, and the greedy capped walk over the rows that beat c keeps
// at least as many rows per group as any cap-valid subset of them does, so it has kept k rows before it reaches c.
// Either way c is not in the capped top-k under s.  The same argument holds for s restricted to any subset of V that
// contains v, so the merge may run in levels over groups of variants, PROVIDED EVERY level de-duplicates, keeps the best
// key per id and caps (a row that enters a later level with less than its best key is one the answer does not hold: the
// rows that shut it out under its best key shut it out under a smaller one).  The per-variant lists must themselves be
// capped: the plain top-k of a variant can consist of one group's rows, and the row the cap promotes is then in no
// list (tests/cpp/grouped_variants_test.cpp shows one).  capped_variants_merge_block below is one block of
// merge_variants_grouped_kernel on the host.
//
// Boosted keys (cs_index_search_variants_boosted_grouped, scan_boosted_grouped.hip): neither argument above reads what a
// key's float is.  They need two things only — every variant orders the rows by a key that is unique per row, and a row's
// merged key is the maximum of its per-variant keys.  Both hold for key_pack(b, id) with b = fl(score(c) * w): w belongs
// to the row, not to the variant, and score and the rounding are monotone in c, so the largest of a row's per-variant b
// is the b of its largest cosine.  Per-variant lists that are capped lists of b (the per-wave lists of the boosted capped
// scan, merged by launch_merge_grouped), merged with de-duplication and the cap at every level, are therefore the capped
// top-k under the best b.  The uncapped boosted variants search is the same merge under a GroupView that caps nothing.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "search_route.hpp"  // kpad_for, kScanWaves

namespace cs {

constexpr uint32_t kNoGroup = 0xFFFFFFFFu;                // CS_NO_GROUP: never capped
constexpr uint32_t kGroupedSlotBytes = 12;                // a list slot: a u64 key and the u32 group beside it
constexpr size_t kGroupedLdsBudget = 64 * 1024;           // LDS per block plan_scan assumes (>= 2 blocks per CU)
constexpr uint32_t kGroupedMergeCap = 4096;               // keys a merge block holds (twice: keys and (group, rank) images)
constexpr size_t kGroupedPartialBudget = (size_t)256 << 20;  // bytes of per-wave lists a search may leave in HBM

struct GroupedPlan {
    uint32_t kpad = 64;        // per-wave list capacity (kpad_for)
    uint32_t qtile = 1;        // queries per scan pass
    uint32_t passes = 1;       // ceil(nq / qtile) (grid.y)
    uint32_t blocks = 1;       // scan grid.x
    bool deep = false;         // one block per CU, twice the rows in flight per wave (one query, a short list)
    size_t lds_bytes = 0;      // dynamic LDS of the scan block: qtile * kScanWaves * kpad * 12
    uint32_t lists = 0;        // partial lists per query: blocks * kScanWaves (one per wave)
    size_t partial_keys = 0;   // nq * lists * k
    uint32_t merge_group = 2;  // lists a merge block takes
    uint32_t merge_levels = 1;
    size_t merge_keys = 0;     // one ping-pong buffer of the multi-level merge (0: one level)
};

inline bool grouped_fast_dim(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }

// Lists per merge block: as many as kGroupedMergeCap keys hold (k <= CS_MAX_K = 1,024 leaves at least four).
inline uint32_t grouped_merge_group(uint32_t k) {
    const uint32_t g = kGroupedMergeCap / (k ? k : 1);
    return g < 2 ? 2 : g;
}

inline uint32_t grouped_merge_levels(uint32_t lists, uint32_t k) {
    const uint32_t G = grouped_merge_group(k);
    uint32_t levels = 1;
    while ((lists = (lists + G - 1) / G) > 1) ++levels;
    return levels;
}

// The capped variants merge (merge_variants_grouped_kernel): a block takes the lists of grouped_merge_group(k) variants,
// so nine lists of more than 455 keys take two levels.  One ping-pong buffer of a multi-level merge, in keys (0: one
// level): the first level's output, ceil(nv / G) lists of k.
inline uint32_t grouped_variants_levels(uint32_t nv, uint32_t k) { return grouped_merge_levels(nv, k); }

inline size_t grouped_variants_tmp_keys(uint32_t nv, uint32_t k) {
    const uint32_t G = grouped_merge_group(k);
    const uint32_t first = (nv + G - 1) / G;
    return first > 1 ? (size_t)first * k : 0;
}

inline GroupedPlan plan_grouped(uint64_t n_rows, uint32_t dim, uint32_t nq, uint32_t k, int num_cus) {
    GroupedPlan p;
    p.kpad = kpad_for(k);
    uint64_t blocks, cap;
    if (grouped_fast_dim(dim)) {
        p.qtile = nq >= 4 ? 4 : (nq >= 2 ? 2 : 1);
        // 12 B per slot where plan_scan counts 8: the tile is lowered until the block stays within the same 64 KiB
        while (p.qtile > 1 && (size_t)p.qtile * kScanWaves * p.kpad * kGroupedSlotBytes > kGroupedLdsBudget) p.qtile >>= 1;
        // the streaming scan's deep shape (scan.hip scan_deep, its default limits); its lists are short, so it always fits
        p.deep = p.qtile == 1 && (k <= 64 || (k <= 128 && n_rows >= 4000000));
        const uint32_t rows_per_tile = p.deep ? (dim == 384 ? 16 : dim == 768 ? 8 : 6) : (dim == 384 ? 8 : 4);
        const uint64_t ntiles = (n_rows + rows_per_tile - 1) / rows_per_tile;
        blocks = (ntiles + kScanWaves - 1) / kScanWaves;
        // blocks per CU: 1 deep and 2 otherwise, as the streaming scan chooses for one or two queries per pass.  Four
        // queries per pass hold 184 to 274 VGPRs here (the group slots cost registers), so two blocks are also what
        // a CU keeps resident of them; the grid-stride loop does not depend on residency.
        cap = (uint64_t)num_cus * (p.deep ? 1 : 2);
    } else {
        p.qtile = 1;
        blocks = (n_rows + kScanWaves - 1) / kScanWaves;  // one wave per row
        cap = (uint64_t)num_cus * 8;
    }
    // every wave leaves a list of k keys: keep them within the budget (fewer blocks scan more rows each)
    const uint64_t by_budget = kGroupedPartialBudget / ((uint64_t)nq * k * sizeof(uint64_t) * kScanWaves);
    if (cap > by_budget) cap = by_budget;
    p.blocks = (uint32_t)std::max<uint64_t>(1, std::min(blocks, cap));
    p.passes = (nq + p.qtile - 1) / p.qtile;
    p.lds_bytes = (size_t)p.qtile * kScanWaves * p.kpad * kGroupedSlotBytes;
    p.lists = p.blocks * kScanWaves;
    p.partial_keys = (size_t)nq * p.lists * k;
    p.merge_group = grouped_merge_group(k);
    p.merge_levels = grouped_merge_levels(p.lists, k);
    const uint32_t first = (p.lists + p.merge_group - 1) / p.merge_group;
    p.merge_keys = first > 1 ? (size_t)nq * first * k : 0;
    return p;
}

// ---- the selection rule on the host ----------------------------------------------------------------

struct GroupedRow {
    uint64_t key;    // packed (cosine, id) key: larger = earlier in (cosine desc, id asc); unique per row
    uint32_t group;
};

// The contract: rows in any order -> the kept rows, best first.
inline std::vector<GroupedRow> capped_topk(std::vector<GroupedRow> rows, uint32_t k, uint32_t m) {
    std::sort(rows.begin(), rows.end(), [](const GroupedRow& a, const GroupedRow& b) { return a.key > b.key; });
    std::vector<GroupedRow> kept;
    for (const GroupedRow& r : rows) {
        if (kept.size() >= k) break;
        if (r.group != kNoGroup) {
            uint32_t have = 0;
            for (const GroupedRow& o : kept) have += o.group == r.group;
            if (have >= m) continue;
        }
        kept.push_back(r);
    }
    return kept;
}

// One step of a wave's list (scan_grouped.hip wave_list_insert_grouped) on the host: `list` holds the capped top-k of
// the rows met so far, `r` is the next row.  A full list lets r in only past its worst key; a saturated group only past
// the group's worst key.
inline void capped_list_step(std::vector<GroupedRow>& list, const GroupedRow& r, uint32_t k, uint32_t m) {
    size_t worst = 0, gworst = 0;
    uint32_t have = 0;
    for (size_t i = 0; i < list.size(); ++i) {
        if (list[i].key < list[worst].key) worst = i;
        if (r.group != kNoGroup && list[i].group == r.group) {
            if (!have || list[i].key < list[gworst].key) gworst = i;
            ++have;
        }
    }
    if (list.size() >= k && !(r.key > list[worst].key)) return;  // the fast-path gate: c > thr
    if (r.group != kNoGroup && have >= m) {
        if (r.key > list[gworst].key) list[gworst] = r;
        return;
    }
    if (list.size() < k) list.push_back(r);
    else list[worst] = r;
}

// One block of the capped merge (merge_topk_grouped_kernel) on the host, step by step as the kernel takes them: sort by
// key; sort (group, position) images so that a group's keys are neighbours, best first; a key whose image has the same
// group per_group places earlier is past the cap; the survivors, in key order, up to k.
inline std::vector<GroupedRow> capped_merge_block(std::vector<GroupedRow> rows, uint32_t k, uint32_t m) {
    std::sort(rows.begin(), rows.end(), [](const GroupedRow& a, const GroupedRow& b) { return a.key > b.key; });
    std::vector<uint64_t> img(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) img[i] = ((uint64_t)rows[i].group << 32) | (0xFFFFFFFFu - (uint32_t)i);
    std::sort(img.begin(), img.end(), [](uint64_t a, uint64_t b) { return a > b; });
    std::vector<bool> cut(rows.size(), false);
    for (size_t i = 0; i < img.size(); ++i) {
        const uint32_t g = (uint32_t)(img[i] >> 32);
        if (g != kNoGroup && i >= m && (uint32_t)(img[i - m] >> 32) == g) cut[0xFFFFFFFFu - (uint32_t)img[i]] = true;
    }
    std::vector<GroupedRow> out;
    for (size_t i = 0; i < rows.size() && out.size() < k; ++i)
        if (!cut[i]) out.push_back(rows[i]);
    return out;
}

// One block of the capped variants merge (merge_variants_grouped_kernel) on the host, step by step as the kernel takes
// them.  `rows` = the keys of the block's variants, one after the other; a packed key carries ~id in its low word, so the
// same id may come with several keys.  The table keeps the largest key of every id (the kernel's LDS hash: one slot per
// id, a 64-bit atomic max), its entries are sorted by key, and from there it is capped_merge_block: the (group, position)
// image sort, the cut, the survivors in key order up to `limit`.
inline std::vector<GroupedRow> capped_variants_merge_block(const std::vector<GroupedRow>& rows, uint32_t limit, uint32_t m) {
    std::vector<GroupedRow> table;  // slot = first sight of the id
    for (const GroupedRow& r : rows) {
        if (r.key == 0) continue;  // an empty slot of a list
        const uint32_t id = ~(uint32_t)r.key;
        size_t slot = 0;
        while (slot < table.size() && ~(uint32_t)table[slot].key != id) ++slot;
        if (slot == table.size()) table.push_back(r);
        else if (r.key > table[slot].key) table[slot] = r;
    }
    return capped_merge_block(table, limit, m);
}

}  // namespace cs
