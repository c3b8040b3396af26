// scope.hpp — cs_scope: a prepared set of chunk ids that lives on the device, belongs to one store and is searched any
// number of times (index.hip cs_index_search_scoped & co.; kernels: scan_masked.hip part 4; plan: masked_plan.hpp).
// A scoped search answers, bit for bit, what the masked search of the same store answers at that moment for a bitmap
// of exactly the scope's ids.
#pragma once

#include <atomic>
#include <mutex>
#include <vector>

#include "common.hpp"
#include "masked_plan.hpp"
#include "scoped_filter_plan.hpp"

// Over one cs_index (index != null) the scope holds, in HBM of the index's device, 8 bytes per id: its ascending ids and
// the row list made from them.  Over a sharded store (shards != null) it holds one such scope per shard over that
// shard's local ids, and nothing else on a device.  A scope over an index that can ever take the int8 filter (the index
// keeps an int8 copy, more than kFilterPhase0 ids: scoped_filter_plan.hpp) additionally keeps, made with the list and
// remade at every refresh: the blocked-rows bitmap (one bit per stored row, HBM), 4 B per 1,024 ids of stride table,
// and on the host (pinned, read back with the length) the list's head, the stride table and the last entry.
struct cs_scope {
    cs_index* index = nullptr;
    cs_shards* shards = nullptr;
    std::vector<cs_scope*> parts;  // per shard (sharded scopes only)
    int device = 0;
    uint64_t n_ids = 0;
    uint32_t* d_ids = nullptr;     // [n_ids] ascending
    uint32_t* d_list = nullptr;    // [n_ids]: the first live_rows entries are the row list
    uint32_t* d_blocks = nullptr;  // [scope_list_blocks(n_ids) + 1]: the id-list pass's offsets; the last word = live_rows
    // pinned: where a making of the list reads back, once, [0] its length and, for a scope with filter tables, [1] the
    // last entry, [2, 1 + table_words) every 1,024th entry, then the first min(n_ids, kScopeHead) entries
    uint32_t* h_len = nullptr;
    uint32_t* d_blocked = nullptr; // [blocked_words]: the blocked-rows bitmap, scope_blocked_words(n_rows) of them in use
    uint32_t* d_table = nullptr;   // [table_words]: the last entry, then every 1,024th (launch_scope_filter_state)
    size_t blocked_words = 0, table_words = 0;
    hipStream_t stream = nullptr;  // the makings of the list run here
    // mu guards the making of the list and the three words below: a search reads them under it, and a refresh
    // publishes them only after its stream has been synchronised
    mutable std::mutex mu;
    uint64_t generation = 0;       // build generation of the index the list was made at; 0 = not made
    uint64_t live_rows = 0;
    uint64_t refreshes = 0;        // makings of the list
    bool filter_state = false;     // the bitmap and the host tables are those of `generation` (guarded by mu as well)
    // the route of the host-buffer searches (cs_scope_set_route) and what they took (cs_scope_route_info)
    std::atomic<int32_t> route{CS_SCOPE_ROUTE_AUTO};
    std::atomic<uint64_t> filter_searches{0}, gathered_searches{0}, overflow_reruns{0};

    cs::ScopeListView list_view() const {  // under mu, filter_state set
        cs::ScopeListView v;
        v.live = live_rows;
        v.last = h_len[1];
        v.stride = h_len + 2;
        v.head = h_len + 1 + table_words;
        return v;
    }
};

namespace cs {

// The id list of a create call, over one index or over shards: at most 2^32 - 1 strictly ascending ids (masked_plan.hpp
// scope_ids_first_unsorted), the message naming the first offending position.
inline int32_t check_scope_ids(const uint32_t* ids, uint64_t n) {
    if (n && !ids) return fail(CS_ERR_BAD_ARG, "ids is null");
    if (n > 0xffffffffull)
        return fail(CS_ERR_BAD_ARG, "a scope holds at most 2^32 - 1 ids (ids are u32), got %llu", (unsigned long long)n);
    const int64_t bad = scope_ids_first_unsorted(ids, n);
    if (bad >= 0)
        return fail(CS_ERR_BAD_ARG, "scope ids must be strictly ascending: ids[%lld] = %u follows ids[%lld] = %u",
                    (long long)bad, ids[bad], (long long)bad - 1, ids[bad - 1]);
    return CS_OK;
}

// The range of a create_range call, over one index or over shards: ids [first_id, first_id + n) inside u32, at most
// 2^32 - 1 of them.
inline int32_t check_scope_range(uint32_t first_id, uint64_t n) {
    if (n > 0xffffffffull)
        return fail(CS_ERR_BAD_ARG, "a scope holds at most 2^32 - 1 ids (ids are u32), got %llu", (unsigned long long)n);
    if ((uint64_t)first_id + n > (1ull << 32))
        return fail(CS_ERR_BAD_ARG, "the range [%u, %u + %llu) ends past 2^32 (ids are u32)", first_id, first_id,
                    (unsigned long long)n);
    return CS_OK;
}

}  // namespace cs
