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

// Over one cs_index (index != null) the scope holds, in HBM of the index's device, 8 bytes per id: its ascending ids and
// the row list made from them.  Over a sharded store (shards != null) it holds one such scope per shard over that
// shard's local ids, and nothing else on a device.
struct cs_scope {
    cs_index* index = nullptr;
    cs_shards* shards = nullptr;
    std::vector<cs_scope*> parts;  // per shard (sharded scopes only)
    int device = 0;
    uint64_t n_ids = 0;
    uint32_t* d_ids = nullptr;     // [n_ids] ascending
    uint32_t* d_list = nullptr;    // [n_ids]: the first live_rows entries are the row list
    uint32_t* d_blocks = nullptr;  // [scope_list_blocks(n_ids) + 1]: the id-list pass's offsets; the last word = live_rows
    uint32_t* h_len = nullptr;     // pinned: where a making of the list reads its length back, once
    hipStream_t stream = nullptr;  // the makings of the list run here
    // mu guards the making of the list and the three words below: a search reads them under it, and a refresh
    // publishes them only after its stream has been synchronised
    mutable std::mutex mu;
    uint64_t generation = 0;       // build generation of the index the list was made at; 0 = not made
    uint64_t live_rows = 0;
    uint64_t refreshes = 0;        // makings of the list
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

}  // namespace cs
