// masked_plan.hpp — the host side of a masked search (scan_masked.hip): an exact top-k over the live rows whose chunk
// ids are set in a caller's bitmap.  Plain C++17, no HIP: tests/cpp/masked_plan_test.cpp checks it on the CPU, and
// index.hip / shards.hip only launch what it returns.
//
// The mask is a bitmap over chunk ids: bit i (bit i & 31 of word i >> 5) allows id i; ids at or above allow_bits are not
// allowed.  A search (index.hip run_masked) then
//   1. bounds the allowed rows by a popcount over the ids the index has issued (allowed_bound): the scan grid is sized
//      from that bound, not from the stored rows, and a bound of 0 launches nothing;
//   2. copies the words that cover those ids to the device (MaskWindow) and compacts the allowed live rows into a row
//      list, ascending (count / scan / scatter, kMaskRowsPerBlock rows per block: no atomic append — the tie rule of
//      the scan's per-wave lists needs every wave to see its rows in ascending order);
//   3. runs the gathered scan over the list (the streaming scan's arithmetic, so the cosines are bit-identical) and the
//      shared key merge.
// A sharded store restates the mask in each shard's local id space first (shard_mask).
#pragma once

#include <cstdint>
#include <vector>

#include "search_route.hpp"  // RouteKnobs, plan_route (prime rows)

namespace cs {

constexpr uint32_t kMaskRowsPerBlock = 4096;  // rows one block of the row-list pass decides (256 threads x 16)

inline uint32_t popcount32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }

// Set bits of allow[] in [lo, hi), hi <= the bits allow[] holds.
inline uint64_t popcount_range(const uint32_t* allow, uint64_t lo, uint64_t hi) {
    if (lo >= hi) return 0;
    uint64_t n = 0;
    const uint64_t w0 = lo >> 5, w1 = (hi - 1) >> 5;
    for (uint64_t w = w0; w <= w1; ++w) {
        uint32_t v = allow[w];
        if (w == w0) v &= ~0u << (lo & 31);
        if (w == w1 && (hi & 31)) v &= (1u << (hi & 31)) - 1u;
        n += popcount32(v);
    }
    return n;
}

// The part of the mask a search reads: ids [lo, hi) with lo a multiple of 32 (the copy starts on a word), hi = the
// smaller of allow_bits and next_id.  The device copy holds words [first_word, first_word + words) of the mask.
struct MaskWindow {
    uint64_t lo = 0, hi = 0;
    uint64_t first_word = 0, words = 0;
};

inline MaskWindow mask_window(uint64_t allow_bits, uint64_t first_id, uint64_t next_id) {
    MaskWindow m;
    m.hi = allow_bits < next_id ? allow_bits : next_id;
    m.lo = (first_id >> 5) << 5;
    if (m.hi <= m.lo) {
        m.lo = m.hi = 0;
        return m;
    }
    m.first_word = m.lo >> 5;
    m.words = (m.hi - m.lo + 31) >> 5;
    return m;
}

// Upper bound of the live allowed rows of an index whose ids are [first_id, next_id) and which stores `stored_rows`
// rows: every stored row has its own id in that range, so no more rows than set bits can pass.
inline uint64_t allowed_bound(const uint32_t* allow, uint64_t allow_bits, uint64_t first_id, uint64_t next_id,
                              uint64_t stored_rows) {
    if (!allow || allow_bits == 0) return 0;
    const uint64_t hi = allow_bits < next_id ? allow_bits : next_id;
    const uint64_t n = popcount_range(allow, first_id, hi);
    return n < stored_rows ? n : stored_rows;
}

inline uint32_t mask_list_blocks(uint64_t stored_rows) {
    return (uint32_t)((stored_rows + kMaskRowsPerBlock - 1) / kMaskRowsPerBlock);
}

// Prime pass in front of the gathered scan: the rule of the streaming route (plan_route) applied to the bound, over the
// first entries of the row list.  0 = none.
inline uint64_t masked_prime_rows(const RouteKnobs& kn, uint64_t bound, uint32_t nq, uint32_t k, uint32_t dim, int cus,
                                  bool prime_supported) {
    SearchShape s;
    s.nq = nq;
    s.k = k;
    s.dim = dim;
    s.n_rows = bound;
    s.cus = cus;
    s.prime = prime_supported;
    return plan_route(kn, s, false).prime_rows;
}

// ---- striped shards (shards.hip) ----------------------------------------------------------------
// Global id g lies in stripe t = g / stripe, which shard t % n holds at local id (t / n) * stripe + g % stripe
// (cs_shards_remove restates ids the same way).

inline uint32_t shard_of(uint64_t g, uint64_t stripe, uint32_t nshards) { return (uint32_t)((g / stripe) % nshards); }
inline uint64_t shard_local_id(uint64_t g, uint64_t stripe, uint32_t nshards) {
    return ((g / stripe) / nshards) * stripe + g % stripe;
}

// Bits [src_off, src_off + n) of src -> bits [dst_off, dst_off + n) of dst (other bits of dst kept; src holds at least
// src_off + n bits, dst dst_off + n).
inline void copy_bits(const uint32_t* src, uint64_t src_off, uint32_t* dst, uint64_t dst_off, uint64_t n) {
    while (n) {
        const uint32_t db = (uint32_t)(dst_off & 31);
        uint32_t take = 32 - db;
        if (take > n) take = (uint32_t)n;
        const uint64_t sw = src_off >> 5;
        const uint32_t sb = (uint32_t)(src_off & 31);
        uint64_t v = src[sw] >> sb;
        if (sb + take > 32) v |= (uint64_t)src[sw + 1] << (32 - sb);
        const uint32_t m = take == 32 ? ~0u : ((1u << take) - 1u);
        uint32_t& d = dst[dst_off >> 5];
        d = (d & ~(m << db)) | (((uint32_t)v & m) << db);
        src_off += take;
        dst_off += take;
        n -= take;
    }
}

// The mask of a store sharded over `nshards` in stripes of `stripe` ids with ids [0, next_id) issued, restated for
// shard `shard` over its local ids: out gets ceil(*out_bits / 32) words, *out_bits = one past the highest local id the
// global mask can allow there (0: nothing on this shard).  Global ids at or above allow_bits stay disallowed.
inline void shard_mask(const uint32_t* allow, uint64_t allow_bits, uint64_t next_id, uint64_t stripe, uint32_t nshards,
                       uint32_t shard, std::vector<uint32_t>& out, uint64_t* out_bits) {
    out.clear();
    *out_bits = 0;
    const uint64_t hi = allow_bits < next_id ? allow_bits : next_id;
    if (!allow || hi == 0 || stripe == 0 || nshards == 0) return;
    const uint64_t nstripes = (hi + stripe - 1) / stripe;
    if (shard >= nstripes) return;
    // the last stripe of this shard below hi bounds the local bits
    const uint64_t t_last = shard + ((nstripes - 1 - shard) / nshards) * nshards;
    const uint64_t g_end = (t_last + 1) * stripe < hi ? (t_last + 1) * stripe : hi;
    *out_bits = shard_local_id(g_end - 1, stripe, nshards) + 1;
    out.assign((size_t)((*out_bits + 31) >> 5), 0u);
    for (uint64_t t = shard; t < nstripes; t += nshards) {
        const uint64_t g0 = t * stripe;
        const uint64_t g1 = g0 + stripe < hi ? g0 + stripe : hi;
        copy_bits(allow, g0, out.data(), shard_local_id(g0, stripe, nshards), g1 - g0);
    }
}

// ---- scopes (index.hip cs_scope, scan_masked.hip launch_scope_rows) -------------------------------
// A scope is a prepared set of chunk ids kept on the device: its strictly ascending ids and the row list made from
// them (the live stored rows that hold those ids, ascending), searched any number of times without a mask.  The list is
// made by one pass over the IDS, kMaskRowsPerBlock of them per block, so its cost follows the scope, not the store.

// ids[0, n) strictly ascending?  -1 when they are, else the first position i >= 1 with ids[i] <= ids[i - 1].
inline int64_t scope_ids_first_unsorted(const uint32_t* ids, uint64_t n) {
    for (uint64_t i = 1; i < n; ++i)
        if (ids[i] <= ids[i - 1]) return (int64_t)i;
    return -1;
}

// Blocks of the id-list pass over a scope of n_ids ids.
inline uint32_t scope_list_blocks(uint64_t n_ids) {
    return (uint32_t)((n_ids + kMaskRowsPerBlock - 1) / kMaskRowsPerBlock);
}

// A row list made at build generation `list_generation` of its index (0: not made yet) is remade by the first search
// that finds the index at another generation: cs_index_build and cs_index_clear advance it, and every other mutation
// un-builds the index, so no search can run between a mutation and the next advance.
inline bool scope_refresh_due(uint64_t list_generation, uint64_t index_generation) {
    return list_generation != index_generation;
}

// The ascending global ids of a scope over a striped store, restated per shard in its local ids: out[s] stays ascending
// (a later stripe of a shard has the larger local ids, and ids inside a stripe keep their order).
inline void shard_scope_ids(const uint32_t* ids, uint64_t n, uint64_t stripe, uint32_t nshards,
                            std::vector<std::vector<uint32_t>>& out) {
    out.assign(nshards, std::vector<uint32_t>());
    if (stripe == 0 || nshards == 0) return;
    for (uint64_t i = 0; i < n; ++i) {
        // (a local id never exceeds its global id, so it fits u32)
        out[shard_of(ids[i], stripe, nshards)].push_back((uint32_t)shard_local_id(ids[i], stripe, nshards));
    }
}

}  // namespace cs
