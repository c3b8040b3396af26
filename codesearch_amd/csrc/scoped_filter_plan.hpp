// scoped_filter_plan.hpp — the host-side plan of a scoped search through the int8 filter (index.hip run_scoped,
// scan_filter.hip launch_scan_split with a prepared plan), and its route.  Plain C++17, no HIP: tests/cpp/
// scoped_filter_plan_test.cpp pins both on the CPU.
//
// plan_filter (filter_plan.hpp) counts in stored rows: phase 0 re-scores the FIRST rows of the store and the phases
// behind it grow geometrically in rows seen.  For a scope the unit is the allowed row, so the boundaries are chosen in
// COUNT space — positions of the scope's ascending row list, with plan_filter's own growth rule over `live` entries —
// and then mapped to ROW space through what the scope keeps on the host: the head of its list and every 1,024th entry.
// The filter kernels then stream the row ranges with the scope's blocked-rows bitmap where the tombstone bitmap goes,
// so only allowed rows become candidates and every allowed row is seen exactly once.
#pragma once

#include <cstdint>

#include "filter_plan.hpp"
#include "search_route.hpp"

namespace cs {

constexpr uint32_t kScopeStride = 1024;                       // the filter kernels' row granule, and the table's stride
constexpr uint32_t kScopeHead = kFilterPhase0 + kScopeStride;  // entries of the list's head kept on the host

// What a scope keeps on the host of its ascending row list (made with the list, cs_scope).
struct ScopeListView {
    uint64_t live = 0;               // entries of the list
    const uint32_t* head = nullptr;  // list[0 .. min(live, kScopeHead))
    const uint32_t* stride = nullptr;  // list[0], list[1024], ...: (live + 1023) / 1024 entries
    uint32_t last = 0;               // list[live - 1]
};

// Entries of the host tables for a list of `live` entries.
inline uint64_t scope_head_entries(uint64_t live) { return live < kScopeHead ? live : kScopeHead; }
inline uint64_t scope_stride_entries(uint64_t live) { return (live + kScopeStride - 1) / kScopeStride; }

// A scope can take the filter at all: the dim has filter kernels and the list outgrows the larger phase 0.  Only
// such a scope holds the bitmap and the host tables.
inline bool scope_filter_capable(uint32_t dim, uint64_t live) {
    return (dim == 384 || dim == 768 || dim == 1024) && live > kFilterPhase0;
}

struct ScopedFilterPlan {
    bool ok = false;     // false: no filter plan for this search — the gathered scan answers it
    uint32_t c0 = 0;     // phase 0 = the list's first c0 entries (= plan.phase0_rows): P <= c0 < P + 1024
    uint64_t b0 = 0;     // ... which are exactly the entries whose row is below b0
    uint64_t span = 0;   // rows the filter phases stream: the last boundary - b0
    // phase[0]: rows [0, b0) of which only the list's first c0 entries are re-scored (no filter launch); phase[1 ..]:
    // row ranges [lo, hi) on the 1,024 granule (the last one ends behind the scope's last row), as plan_filter's
    FilterPlan plan;
    uint8_t src[kMaxFilterPhases] = {};  // plan.phase[i] took kernel, tiles and refine blocks from plan_filter's phase src[i]
};

// Words of the blocked-rows bitmap of a store of n_rows rows: one bit per row, rounded up to whole 1,024-row granules
// (the filter kernels work in 128- and 256-row tiles: a tile that straddles the store's end finds blocked bits there).
inline uint64_t scope_blocked_words(uint64_t n_rows) { return (n_rows + kScopeStride - 1) / kScopeStride * (kScopeStride / 32); }

inline uint64_t scope_round_up(uint64_t v) { return (v + kScopeStride - 1) / kScopeStride * kScopeStride; }
inline uint64_t scope_round_down(uint64_t v) { return v / kScopeStride * kScopeStride; }

// The plan of one scoped search of nq queries, top-k, over a store of n_rows rows of `dim` whose int8 copy holds
// q8_rows rows (complete 128-row tiles; fewer than 128 rows lie behind it).
inline ScopedFilterPlan plan_scoped_filter(uint32_t dim, uint64_t n_rows, const ScopeListView& L, uint32_t nq, uint32_t k,
                                           uint64_t q8_rows, bool have_query_planes, int cus, const FilterKnobs& kn) {
    ScopedFilterPlan s;
    if (!scope_filter_capable(dim, L.live) || !L.head || !L.stride || q8_rows <= kFilterPhase0) return s;
    // kernel, queries per tile, query tiles, plane choice, refine blocks and the count boundaries: plan_filter's own,
    // over `live` rows all of which the int8 copy covers
    const FilterPlan t = plan_filter(dim, L.live, nq, k, ~(uint64_t)0, have_query_planes, cus, kn);
    if (!t.use_q8 || t.nphases < 2) return s;
    const uint32_t P = t.phase0_rows;  // 3,072, or 1,024 above 32 queries (live > 3,072)
    s.b0 = scope_round_up((uint64_t)L.head[P - 1] + 1);
    const uint64_t head_n = scope_head_entries(L.live);
    uint32_t c0 = P;
    while (c0 < head_n && L.head[c0] < s.b0) ++c0;  // fewer than 1,024 rows lie between list[P - 1] and b0
    if (c0 >= L.live) return s;                     // everything fits phase 0
    if (c0 >= head_n) return s;                     // (cannot happen: c0 < P + 1024 <= kScopeHead)
    s.c0 = c0;
    const int cus8 = cus >= 8 ? cus / 8 * 8 : 256;
    FilterPlan& p = s.plan;
    p.use_q8 = true;
    p.two_planes = t.two_planes;
    p.phase0_rows = c0;
    FilterPhase& f0 = p.phase[p.nphases++];
    f0 = t.phase[0];  // kernel None, its refine blocks
    f0.lo = 0;
    f0.hi = f0.filter_hi = s.b0;
    f0.tail_lo = f0.tail_hi = 0;
    uint64_t done = s.b0;
    for (uint32_t i = 1; i < t.nphases; ++i) {
        const uint64_t c = t.phase[i].hi;  // count boundary: a multiple of 1,024, or live
        uint64_t b;
        if (c >= L.live) {
            b = scope_round_up((uint64_t)L.last + 1);  // the end of the granule that holds the scope's last row
            if (b > n_rows) b = n_rows;
        } else {
            if (c % kScopeStride) return ScopedFilterPlan();  // (a laboratory growth knob off the granule)
            b = scope_round_down(L.stride[c / kScopeStride]);
        }
        if (b <= done) continue;  // no entry of the list lies in it
        s.src[p.nphases] = (uint8_t)i;
        FilterPhase& f = p.phase[p.nphases++];
        f = t.phase[i];
        f.lo = done;
        f.hi = b;
        const uint64_t q_hi = b < q8_rows ? b : q8_rows;
        f.filter_hi = q_hi;
        f.grid = f.slots = 0;
        if (q_hi <= f.lo) {  // wholly behind the copy's last complete tile
            f.kernel = FilterKernel::None;
            f.nqt = f.qtiles = 0;
        } else if (f.kernel == FilterKernel::Q8Tile256) {
            f.slots = filter_grid_slots((uint32_t)((q_hi - f.lo + 255) / 256), (nq + 255) / 256);
            f.grid = f.slots < (uint32_t)cus8 ? f.slots : (uint32_t)cus8;
        } else if (f.kernel == FilterKernel::Q8Rq || f.kernel == FilterKernel::Q8Rq1) {
            f.grid = filter_resident_grid(((q_hi - f.lo) / 128 + 1) / 2, f.qtiles, cus8);
        } else if (f.kernel == FilterKernel::Q8Rw || f.kernel == FilterKernel::Q8Rw2) {
            f.grid = filter_resident_grid((q_hi - f.lo) / 128, f.qtiles, cus8);
        } else {
            return ScopedFilterPlan();  // not an int8 kernel: no scoped filter
        }
        f.tail_lo = f.lo > q8_rows ? f.lo : q8_rows;
        f.tail_hi = f.hi > f.tail_lo ? f.hi : f.tail_lo;
        done = b;
    }
    if (p.nphases < 2) return ScopedFilterPlan();
    s.span = done - s.b0;
    s.ok = true;
    return s;
}

// ---- route -----------------------------------------------------------------------------------------

// One scoped host-buffer search as its route sees it.
struct ScopedRouteIn {
    int mode = CS_SCOPE_ROUTE_AUTO;  // cs_scope_set_route
    bool q8_serves = false;          // (a) the index's int8 copy serves
    bool plan_ok = false;            // plan_scoped_filter found a plan (supported dim, more than phase 0 holds)
    uint64_t live = 0, span = 0;     // the list's entries; the rows its filter phases stream
};

// Does it want the filter?  (Whether the int8 query planes fit is asked afterwards, as run_search asks it.)
//   (a) the int8 copy serves and a plan exists — never waived;
//   (b) route_wants_filter for the shape with the scope's live rows in place of n_rows (`shape.n_rows` = live);
//   (c) the rows streamed are at most scope_filter_max_span(nq) x live.
// CS_SCOPE_ROUTE_FILTER waives (b) and (c); CS_SCOPE_ROUTE_GATHER never takes the filter.
inline bool scoped_wants_filter(const RouteKnobs& kn, const SearchShape& shape, const ScopedRouteIn& in) {
    if (in.mode == CS_SCOPE_ROUTE_GATHER || !in.q8_serves || !in.plan_ok) return false;
    if (in.mode == CS_SCOPE_ROUTE_FILTER) return true;
    if (!route_wants_filter(kn, shape, in.q8_serves)) return false;
    return (double)in.span <= kn.scope_filter_max_span(shape.nq) * (double)in.live;
}

}  // namespace cs
