// similar_sources.hpp — the host side of the similar-chunk search (cs_index_search_similar; kernels: scan_similar.hip):
// what a call's source ids mean under the ledger and the group table.  Plain C++17, no HIP, one pure function:
// tests/cpp/similar_sources_test.cpp walks it against a naive restatement on the CPU, and index.hip only copies and
// launches what it answers.
//
// For source ids[q]:
//   row       the stored row that carries the id — wherever a reclaiming build has moved it;
//   live      an id never issued has no row; an id issued and deleted has a tombstoned row, or none once reclaimed: both
//             are refused, with different texts, and the first offending position is reported;
//   excluded  CS_SIMILAR_EXCLUDE_NONE   nothing;
//             CS_SIMILAR_EXCLUDE_SELF   the id itself;
//             CS_SIMILAR_EXCLUDE_GROUP  the id itself, and its group when that is not CS_NO_GROUP (ids past the end of the
//                                       table are CS_NO_GROUP: with no group assigned this mode is EXCLUDE_SELF).
#pragma once

#include "index_ledger.hpp"

namespace cs {

// "no id": ids stop at 2^32 - 2 (IndexLedger::can_append keeps next_id <= 2^32 - 1), so no row carries it
constexpr uint32_t kNoExcludedId = 0xFFFFFFFFu;

enum class SourceFault : uint32_t { None = 0, NeverIssued = 1, Deleted = 2 };
struct SourceCheck {
    SourceFault fault;
    uint32_t at;  // position in ids of the first offending one (fault != None)
};

inline bool similar_mode_ok(int32_t exclude) { return exclude >= CS_SIMILAR_EXCLUDE_NONE && exclude <= CS_SIMILAR_EXCLUDE_GROUP; }

// The group of an id as the kernels read the table: entry id - id_base, CS_NO_GROUP past its end.
inline uint32_t similar_group_of_id(const IndexLedger& ledger, const GroupTable& groups, uint32_t id) {
    const uint64_t e = (uint64_t)id - ledger.id_base();
    return (id >= ledger.id_base() && e < groups.size()) ? groups.data()[e] : CS_NO_GROUP;
}

// Resolves ids[0, nq) under mode `exclude` (similar_mode_ok).  Every id live: rows[q], ex_ids[q], ex_groups[q] are
// written for every q (each array optional: pass null for a check alone) and fault = None.  Otherwise the first offending
// position is returned and the arrays hold nothing a caller may use.
inline SourceCheck resolve_similar_sources(const IndexLedger& ledger, const GroupTable& groups, const uint32_t* ids,
                                           uint32_t nq, int32_t exclude, uint32_t* rows, uint32_t* ex_ids,
                                           uint32_t* ex_groups) {
    const std::vector<uint32_t>& dead = ledger.dead_words();
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t id = ids[q];
        if (!ledger.issued(id)) return SourceCheck{SourceFault::NeverIssued, q};
        const uint64_t row = ledger.row_of(id);
        if (row == kNoRow) return SourceCheck{SourceFault::Deleted, q};                           // reclaimed
        if ((dead[(size_t)(row / 32)] >> (row % 32)) & 1u) return SourceCheck{SourceFault::Deleted, q};  // tombstoned
        if (rows) rows[q] = (uint32_t)row;  // rows < 2^32: every stored row carries a u32 id of its own
        if (ex_ids) ex_ids[q] = exclude == CS_SIMILAR_EXCLUDE_NONE ? kNoExcludedId : id;
        if (ex_groups) ex_groups[q] = exclude == CS_SIMILAR_EXCLUDE_GROUP ? similar_group_of_id(ledger, groups, id) : CS_NO_GROUP;
    }
    return SourceCheck{SourceFault::None, 0};
}

}  // namespace cs
