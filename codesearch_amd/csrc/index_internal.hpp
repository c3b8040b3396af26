// index_internal.hpp — what index.hip (the store and its searches) and index_joins.hip (the similar-pairs and
// similar-clusters calls) share: the handle, the buffer helpers, and the few index.hip functions a join calls.
#pragma once

#include <atomic>
#include <map>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "index_ledger.hpp"
#include "scan.hpp"
#include "scope.hpp"

namespace cs {

struct EventTriple {
    hipEvent_t e0, e1, e2;
};

// Frees p (pinned host memory when `pinned`) and, for n > 0, allocates n elements in its place: null on failure.
template <class T>
hipError_t realloc_buf(T*& p, size_t n, bool pinned = false) {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    if (!n) return hipSuccess;
    return pinned ? hipHostMalloc(&p, n * sizeof(T)) : hipMalloc(&p, n * sizeof(T));
}
template <class... T>
void free_bufs(bool pinned, T*&... p) {
    ((void)realloc_buf(p, 0, pinned), ...);
}
// p holds at least n elements afterwards; cap = how many it holds (0 after a failed allocation)
template <class T>
int32_t reserve_buf(T*& p, size_t& cap, size_t n, bool pinned = false) {
    if (n <= cap) return CS_OK;
    cap = 0;
    CS_HIP(realloc_buf(p, n, pinned));
    cap = n;
    return CS_OK;
}

struct Workspace;          // index.hip: a search's scratch
struct PairsWorkspace;     // index_joins.hip: a similar-pairs call's
struct ClustersWorkspace;  // index_joins.hip: a similar-clusters call's

}  // namespace cs

struct cs_index {
    int device = 0;
    int num_cus = 256;
    uint32_t dim = 0;
    uint64_t capacity = 0;   // rows allocated
    // ids, stored rows and tombstones (index_ledger.hpp): the host's side of everything below that is numbered by them
    cs::IndexLedger ledger;
    // the device copy of the ledger's row -> id table, once it is compacted: cs_index_build uploads the rows that are new
    uint32_t* d_ids = nullptr;
    uint64_t ids_cap = 0, ids_uploaded = 0;
    uint32_t compact_dead_pct = 10;  // cs_index_build reclaims from this share of tombstones on (CS_INDEX_COMPACT_DEAD_PCT; 0 = never)
    uint64_t compactions = 0;
    // (d_ids of a compacted index is null only while it stores no row: cs_index_build uploads the table before any search)
    cs::RowIds row_ids() const { return cs::RowIds(ledger.id_base(), ledger.compacted() ? d_ids : nullptr); }
    // Groups of the grouped search (scan_grouped.hip).  The device copy is brought up to date under groups_mu by the
    // first grouped search that finds it dirty (ensure_groups); searches read it only.
    cs::GroupTable groups;
    uint32_t* d_groups = nullptr;
    uint64_t groups_cap = 0;  // elements allocated on the device
    std::mutex groups_mu;
    // Classes of the boosted search (scan_boosted.hip): the group table's sibling, 2 B per id, brought up to date under
    // classes_mu by the first boosted search that finds it dirty (ensure_classes); searches read it only.
    cs::ClassTable classes;
    uint16_t* d_classes = nullptr;
    uint64_t classes_cap = 0;  // elements allocated on the device
    std::mutex classes_mu;
    float* d_corpus = nullptr;
    uint32_t* d_dead = nullptr;  // bitmap over rows, sized for `capacity`
    float* d_norms = nullptr;    // |row| for rows [0, normed_rows) (batched-query path)
    uint64_t normed_rows = 0;
    // unit rows [0, split_rows) as f16 [row][dim]: the filter operand of the batched path WHEN the int8 copy does not
    // serve (no int8 copy, retired by its spread or by strikes, <= 1024 rows).  Built on demand (ensure_f16): an index
    // whose int8 copy serves holds 5 bytes per element (f32 + int8), not 7, and its builds skip the conversion.
    _Float16* d_split = nullptr;
    uint64_t split_rows = 0, split_cap = 0;
    bool use_split = false;
    bool f16_eager = false;    // CS_FILTER_F16_EAGER=1 (or an A/B knob that needs both copies): build it at every cs_index_build
    bool f16_failed = false;   // no room for it: searches stay on the int8 copy / the exact paths (reset by clear())
    std::mutex filter_mu;      // guards the on-demand build (searches are re-entrant)
    // int8 filter copy (scan_filter.hip): complete 128-row tiles [0, q8_rows / 128), a quarter of the f32 bytes
    int8_t* d_q8 = nullptr;
    float4* d_tmeta = nullptr;
    float* d_mu = nullptr;   // [dim] mean unit row of the first build: the copy holds u - mu (fixed until clear())
    uint64_t q8_rows = 0;
    bool use_q8 = false;
    // The int8 copy stops being the filter operand (the f16 copy takes over, results unchanged) when the data defeat its
    // error band: at build, when the tiles' scales say so (outlier coordinates: q8_spread), and at run time after two
    // searches through it overflowed a candidate buffer.  clear() resets both.
    std::atomic<bool> q8_active{true};
    std::atomic<uint32_t> q8_strikes{0}, q8_searches{0};
    // a strike; the copy is retired once there are two and they are more than one in sixteen of its searches
    void q8_strike() {
        const uint32_t s = q8_strikes.fetch_add(1) + 1;
        if (s >= 2 && (uint64_t)s * 16 >= q8_searches.load()) q8_active.store(false);
    }
    float q8_spread = 0.0f;      // median over tiles of max |u - mu| * sqrt(dim) at the last build (isotropic rows: ~4.4)
    float q8_max_spread = 7.0f;  // CS_FILTER_INT8_MAX_SPREAD
    float filter_margin = 0.0f;  // scan_filter.hip: bound of the f16 filter's error for this dim
    cs::RouteKnobs route;  // search_route.hpp: the thresholds of plan_route (route_knobs_from_env)
    uint64_t batched_searches = 0, batched_fallbacks = 0, q8_reruns = 0;
    // The similar-chunk search's route (similar_route.hpp; cs_index_set_similar_route, CS_SIMILAR_ROUTE) and its own counters
    // (cs_index_similar_route_info): unscoped calls the filter answered — those whose candidate buffer overflowed and that
    // the similar scan then answered among them, counted again in the fallbacks — and unscoped calls the scan answered.
    // The counters above and the int8 copy's strikes do not move for similar calls.
    std::atomic<int32_t> similar_route{CS_SIMILAR_ROUTE_AUTO};
    std::atomic<uint64_t> similar_filter_searches{0}, similar_scan_searches{0}, similar_filter_fallbacks{0};
    bool built = false;
    // Build generation: cs_index_build and cs_index_clear advance it.  Every other mutation un-builds the index and a
    // search needs a build, so whatever a scope derived from the stored rows (its row list, scope.hpp) is current
    // exactly while the generation is the one it was derived at.
    std::atomic<uint64_t> build_gen{1};
    // streams of OTHER devices that carry unfinished appends into this corpus (index_append_from: an encoder replica on
    // another GPU writing its rows over xGMI); hipDeviceSynchronize on this device does not wait for them
    // peer appends in flight: ONE event per (source device, stream), re-recorded by every append on that stream (a later
    // record covers the stream's earlier copies), so an ingest of millions of rows in mini-batches keeps a handful of events.
    // CONTRACT (include/codesearch_gpu.h, cs_shards_add_device / cs_embedders_index_*): a stream that carried an append must
    // stay alive until the next build / search / read of this index has drained it — a destroyed stream whose handle value is
    // handed out again would have its slot's event re-recorded on the NEW stream and the old copies would go untracked
    struct ForeignAppend { int device; hipStream_t stream; hipEvent_t done; };
    std::vector<ForeignAppend> foreign_appends;

    std::mutex mu;  // guards the pools below (search is re-entrant)
    std::vector<cs::Workspace*> pool;
    std::vector<cs::PairsWorkspace*> pairs_pool;  // cs_index_similar_pairs' scratch, one set per call in flight
    std::vector<cs::ClustersWorkspace*> clusters_pool;  // cs_index_similar_clusters', likewise
    // device-API scratch: one set per (stream, calling thread) — stream order makes reuse safe within a
    // thread, and two threads sharing a stream (e.g. both on the null stream) never share a set
    std::map<std::pair<hipStream_t, std::thread::id>, cs::Workspace*> by_stream;
    bool profile = false;
    std::vector<cs::EventTriple> pending;
    double scan_ms = 0.0, merge_ms = 0.0;
    uint64_t scan_launches = 0;
};

namespace cs {

// ---- index.hip -------------------------------------------------------------------------------------------------------
bool q8_serves(const cs_index* h);
bool ensure_f16(cs_index* h);
int32_t ensure_groups(cs_index* h, uint32_t per_group, GroupView* gv);
int32_t check_search(const cs_index* h, uint32_t nq, uint32_t dim, uint32_t k);
int32_t check_scope_handle(const cs_index* h, const cs_scope* sc);
int32_t scope_ready(cs_index* h, cs_scope* sc, uint64_t* live, ScopedFilterPlan* fp = nullptr, uint32_t nq = 0, uint32_t k = 0);

// ---- index_joins.hip -------------------------------------------------------------------------------------------------
// cs_index_destroy: frees the two join pools (their types are index_joins.hip's); the index's device is current
void free_join_pools(cs_index* h);

}  // namespace cs
