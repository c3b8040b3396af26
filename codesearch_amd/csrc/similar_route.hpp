// similar_route.hpp — the route of a similar-chunk search (index.hip search_similar): the f32 streaming scan under the
// exclusions (scan_similar.hip), or the int8 / f16 filter with the similar refine and fold (scan_similar_filter.hip).  Both
// return the same bits; the route is a matter of cost only.  Plain C++17, no HIP: tests/cpp/similar_route_test.cpp pins the
// routes on the CPU, and search_similar only launches what plan_similar_route returns.
// This is the UNSCOPED call's route.  The scoped call (index.hip run_similar_scoped) has no logic here: its route is its
// scope's (cs_scope_set_route), decided by scope_ready with scoped_wants_filter (scoped_filter_plan.hpp) exactly as for the
// ordinary scoped search, and the functions below keep answering Scan for scoped == true.
#pragma once

#include <cstdint>

#include "../../include/codesearch_gpu.h"  // CS_SIMILAR_ROUTE_*
#include "search_route.hpp"

namespace cs {

enum class SimilarRoute : uint8_t { Scan, Filter };

// The filter kernels' widths (scan_filter.hip split_scan_supported, restated: this header carries no HIP).
inline bool similar_filter_dim(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }

// Step 1: does this call look for a filter copy at all?  `s` describes the call as an ordinary search of s.nq queries that
// already sit in device memory (the gathered source rows do: s.pinned is false) at s.k over every stored row.
//   AUTO    exactly when route_wants_filter says that ordinary search would — the gathered rows ARE such queries, and the
//           filter's work does not depend on what the refine drops — at a width the filter kernels have, outside a scope.
//   FILTER  the size thresholds of route_wants_filter are dropped (query count, the few-queries window, the one-query row
//           counts, the single-query route); the preconditions stay: filter copies are kept (use_split), the row norms cover
//           every row, the width, no scope.
//   SCAN    never.
// A scoped call always answers false: cs_index_set_similar_route does not govern the scoped similar search.
inline bool similar_wants_filter(const RouteKnobs& kn, const SearchShape& s, bool q8_serves, bool scoped, int32_t forced) {
    if (forced == CS_SIMILAR_ROUTE_SCAN || scoped || !similar_filter_dim(s.dim) || s.pinned) return false;
    if (forced == CS_SIMILAR_ROUTE_FILTER) return s.use_split && s.normed;
    return route_wants_filter(kn, s, q8_serves);
}

// Step 2: the route, given whether index.hip obtained a filter copy the way run_search obtains it (the int8 copy when it
// serves and its query planes fit, else the f16 copy through ensure_f16) and room for the filter's buffers — have_copy is
// false when any of that answered "no room", and only ever true when similar_wants_filter said so.  The filter is taken
// exactly when plan_route would then answer SearchPath::Filter.  BatchedExact is never taken: there is no exact-MFMA similar
// route, so a call plan_route would send there scans.
inline SimilarRoute plan_similar_route(const RouteKnobs& kn, const SearchShape& s, bool q8_serves, bool have_copy, bool scoped,
                                       int32_t forced) {
    if (!have_copy || !similar_wants_filter(kn, s, q8_serves, scoped, forced)) return SimilarRoute::Scan;
    return plan_route(kn, s, true).path == SearchPath::Filter ? SimilarRoute::Filter : SimilarRoute::Scan;
}

}  // namespace cs
