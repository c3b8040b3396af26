// index_ledger.hpp — the host-side ledger of an index (index.hip): which id each stored row carries, which row holds an
// id, which rows are dead, which ids are spent — and the group and the class of every id (scan_grouped.hip, scan_boosted.hip).  Plain C++17, no HIP:
// tests/cpp/index_ledger_test.cpp walks it against a model on the CPU, and index.hip only allocates, copies and launches
// what it answers.
//
// Reclaiming deleted rows (store.rs:548-610: arroy drops deleted items at the next build; the incremental `index` deletes a
// changed file's chunks and re-inserts them, src/index/mod.rs:525,544 — a store re-indexed daily would otherwise only grow):
// when at least dead_pct % of the stored rows are tombstones, cs_index_build rewrites corpus (norms and the filter copies
// are rebuilt from it) without them.  Ids stay what they were: once `compacted`, the row -> id table (and its device copy)
// = the id of each stored row, ascending; until then id = id_base + row and the table is empty.
// (CS_INDEX_COMPACT_DEAD_PCT, default 10; 0 = never.)  The flag, not an empty table, says which numbering holds: a reclaim
// of an index whose rows are all deleted leaves no row and so an empty table, yet the ids it has issued are spent (never
// reused, store.rs:101) and the rows appended next continue from n_ids, not from row 0.  Only clear() returns to the
// identity numbering.  row_of() (id -> row) and id_at() (row -> id) are the two places that choose an id's row or a row's
// id by the flag; append() and id_run() read it only to extend the table or to skip a walk that the identity numbering
// makes trivial.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/codesearch_gpu.h"  // CS_NO_GROUP, CS_NO_CLASS

namespace cs {

constexpr uint64_t kNoRow = ~0ull;  // row_of / id_run: the id names no stored row

class IndexLedger {
public:
    explicit IndexLedger(uint32_t id_base = 0) : id_base_(id_base) {}

    uint32_t id_base() const { return id_base_; }
    uint64_t issued_ids() const { return n_ids_; }                     // ids issued so far: [id_base, next_id)
    uint32_t next_id() const { return id_base_ + (uint32_t)n_ids_; }   // ids are never reused (store.rs:101)
    uint64_t stored() const { return n_rows_; }                        // rows in storage, tombstoned ones included
    uint64_t removed() const { return n_removed_; }                    // tombstoned rows still in storage
    uint64_t live() const { return n_rows_ - n_removed_; }
    bool compacted() const { return compacted_; }

    // ids are u32 (store.rs:97): n more fit?
    bool can_append(uint64_t n) const { return (uint64_t)id_base_ + n_ids_ + n <= 0xffffffffull; }

    // n rows appended to storage: they carry the next n ids.  Returns the first.
    uint32_t append(uint64_t n) {
        const uint32_t first = next_id();
        if (compacted_)  // the new rows' ids join the row -> id table (uploaded by the next build)
            for (uint64_t i = 0; i < n; ++i) ids_.push_back(first + (uint32_t)i);
        n_ids_ += n;
        n_rows_ += n;
        dead_.resize(words(n_rows_), 0u);
        return first;
    }

    bool issued(uint32_t id) const { return id >= id_base_ && (uint64_t)id - id_base_ < n_ids_; }

    // The stored row that carries `id`: kNoRow for an id never issued, or deleted and reclaimed.  (A tombstoned row that
    // is still in storage has a row.)
    uint64_t row_of(uint32_t id) const {
        if (!issued(id)) return kNoRow;
        if (!compacted_) return (uint64_t)id - id_base_;  // n_rows = n_ids until the first reclaim
        const auto it = std::lower_bound(ids_.begin(), ids_.end(), id);  // the table is ascending
        return it != ids_.end() && *it == id ? (uint64_t)(it - ids_.begin()) : kNoRow;
    }

    // Tombstones the rows of ids[0, n).  Returns how many are newly dead: an id without a row (row_of) or already dead
    // — earlier in this list included — is not counted (del_item fails -> not counted, store.rs:594).
    uint64_t remove(const uint32_t* ids, uint64_t n) {
        uint64_t cnt = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t row = row_of(ids[i]);
            if (row == kNoRow || dead(row)) continue;
            dead_[word(row)] |= bit(row);
            ++cnt;
        }
        n_removed_ += cnt;
        return cnt;
    }

    // cs_index_build reclaims the tombstoned rows now?
    bool wants_reclaim(uint32_t dead_pct) const {
        return dead_pct && n_removed_ && n_removed_ * 100 >= (uint64_t)dead_pct * n_rows_;
    }

    // Reclaim, part 1 (any number of times, chunk by chunk): the live ones of the stored rows [c0, c1), relative to c0,
    // appended to out.
    void survivors(uint64_t c0, uint64_t c1, std::vector<uint32_t>& out) const {
        for_live(c0, c1, [&](uint64_t r) { out.push_back((uint32_t)(r - c0)); });
    }

    // Reclaim, part 2 (once every survivor has moved to the front of storage, in order): the table keeps the survivors'
    // ids, no row is dead, and the numbering is the table's from here on — also when no row is left.
    void commit_reclaim() {
        std::vector<uint32_t> kept;
        kept.reserve((size_t)live());
        for_live(0, n_rows_, [&](uint64_t r) { kept.push_back(id_at(r)); });
        ids_.swap(kept);
        compacted_ = true;
        n_rows_ = ids_.size();
        n_removed_ = 0;
        dead_.assign(words(n_rows_), 0u);
    }

    // The stored rows that carry the ids id_base + first_rel, + 1, ... : the row of the first and how many of the
    // following rows (at most n in all) carry the consecutive ids.  row = kNoRow when the first id has no row.
    struct Run { uint64_t row, len; };
    Run id_run(uint64_t first_rel, uint64_t n) const {
        const uint64_t row = first_rel < n_ids_ ? row_of(id_base_ + (uint32_t)first_rel) : kNoRow;
        if (row == kNoRow) return Run{kNoRow, 0};
        const uint64_t room = std::min(n, n_rows_ - row);
        if (!compacted_) return Run{row, room};  // neighbours in id are neighbours in storage: no walk
        uint64_t len = 0;
        while (len < room && id_at(row + len) == id_at(row) + len) ++len;
        return Run{row, len};
    }

    // For the uploads: the tombstone bitmap (bit row & 31 of word row / 32; ceil(stored / 32) words, bits past the
    // stored rows zero) and the row -> id table (stored() entries once compacted, else empty).
    const std::vector<uint32_t>& dead_words() const { return dead_; }
    const uint32_t* ids_data() const { return ids_.data(); }

    // store.rs:701 next_id = 0: no rows, no ids spent, the identity numbering at id_base again
    void clear() { *this = IndexLedger(id_base_); }

private:
    static size_t words(uint64_t rows) { return (size_t)((rows + 31) / 32); }
    static size_t word(uint64_t row) { return (size_t)(row / 32); }
    static uint32_t bit(uint64_t row) { return 1u << (row % 32); }
    bool dead(uint64_t row) const { return (dead_[word(row)] & bit(row)) != 0; }
    uint32_t id_at(uint64_t row) const { return compacted_ ? ids_[(size_t)row] : id_base_ + (uint32_t)row; }

    // f(row) for the live rows of [r0, r1), ascending: a word of the bitmap at a time
    template <class F>
    void for_live(uint64_t r0, uint64_t r1, F&& f) const {
        for (uint64_t base = r0 / 32 * 32; base < r1; base += 32) {
            uint32_t alive = ~dead_[word(base)];
            if (base < r0) alive &= ~0u << (r0 - base);
            if (r1 - base < 32) alive &= (1u << (r1 - base)) - 1u;
            for (; alive; alive &= alive - 1) f(base + (uint64_t)__builtin_ctz(alive));
        }
    }

    uint32_t id_base_;
    uint64_t n_ids_ = 0, n_rows_ = 0, n_removed_ = 0;
    bool compacted_ = false;
    std::vector<uint32_t> ids_;   // row -> id once compacted, ascending
    std::vector<uint32_t> dead_;  // tombstone bitmap over the stored rows
};

// A value of every id — its group (the grouped search, scan_grouped.hip: GroupTable) or its class (the boosted search,
// scan_boosted.hip: ClassTable): entry id - id_base for the ids assigned so far (shorter than the issued ids when ids
// were appended since: those are NONE), empty = none assigned — and what a device copy of device_len entries has not seen
// of it.  The values are a property of ids and go when the ids go (clear()).
template <class T, T NONE>
class IdTable {
public:
    // values[i] becomes the value of ids[i] (NONE un-assigns it).  An id the ledger never issued: nothing is changed
    // and its position in ids is returned; -1 otherwise.  Ledger: issued(id) and id_base() — an index's IndexLedger, or
    // the sharded store's count of ids issued (shards.hip).
    template <class Ledger>
    int64_t set(const uint32_t* ids, const T* values, uint64_t n, const Ledger& ledger) {
        uint32_t top = 0;  // the highest entry touched
        for (uint64_t i = 0; i < n; ++i) {
            if (!ledger.issued(ids[i])) return (int64_t)i;
            top = std::max(top, ids[i] - ledger.id_base());
        }
        if (n && values_.size() <= top) values_.resize((size_t)top + 1, NONE);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t e = ids[i] - ledger.id_base();
            T& g = values_[e];
            if (g == values[i]) continue;
            assigned_ += (uint64_t)(values[i] != NONE) - (uint64_t)(g != NONE);
            g = values[i];
            dirty_lo_ = dirty_hi_ > dirty_lo_ ? std::min<uint64_t>(dirty_lo_, e) : e;
            dirty_hi_ = std::max<uint64_t>(dirty_hi_, (uint64_t)e + 1);
        }
        return -1;
    }

    uint64_t assigned() const { return assigned_; }  // entries != NONE
    uint64_t size() const { return values_.size(); }
    const T* data() const { return values_.data(); }

    // Entries [*lo, *hi) the device copy has not seen: the ones changed since uploaded(), and the ones past its end.
    // false: it is up to date.
    bool pending(uint64_t* lo, uint64_t* hi) const {
        *lo = dirty_lo_;
        *hi = dirty_hi_;
        if (values_.size() > device_len_) {
            *lo = dirty_hi_ > dirty_lo_ ? std::min(dirty_lo_, device_len_) : device_len_;
            *hi = values_.size();
        }
        return *hi > *lo;
    }
    // The device copy now holds entries [0, n) as they are here.  (0: it holds nothing, e.g. it was reallocated.)
    void uploaded(uint64_t n) {
        device_len_ = n;
        dirty_lo_ = dirty_hi_ = 0;
    }

    void clear() { *this = IdTable(); }

private:
    std::vector<T> values_;
    uint64_t assigned_ = 0;
    uint64_t dirty_lo_ = 0, dirty_hi_ = 0;  // entries [lo, hi) changed since uploaded()
    uint64_t device_len_ = 0;
};
using GroupTable = IdTable<uint32_t, CS_NO_GROUP>;            // 4 B per id issued
using ClassTable = IdTable<uint16_t, (uint16_t)CS_NO_CLASS>;  // 2 B per id issued

}  // namespace cs
