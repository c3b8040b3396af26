// index_joins.hip — the joins of a store's rows with each other: cs_index_similar_pairs and cs_index_similar_clusters over the
// whole store, their _scoped forms over the row lists of one or two scopes, and the _info calls.  Host code only: the kernels
// are scan_pairs.hip, scan_pairs_scoped.hip, scan_clusters.hip and scan_clusters_scoped.hip, the plans pairs_plan.hpp,
// pairs_scoped_plan.hpp, clusters_plan.hpp and clusters_scoped_plan.hpp.  The four calls share one frame, each step of which
// is stated once below: the workspace and its lease, the argument checks, the f16 operand (the whole store's, or two packed
// scopes), the timed launch, the pairs calls' band loop and tail, the clusters calls' walk and tail.
#include <algorithm>
#include <chrono>
#include <mutex>
#include <vector>

#include <cstdlib>

#include "clusters_plan.hpp"
#include "clusters_scoped_plan.hpp"
#include "index_internal.hpp"
#include "pairs_plan.hpp"
#include "pairs_scoped_plan.hpp"

namespace cs {

// Scratch of a join call: a stream, events and counters of its own, pooled per index — a call never touches a search's
// Workspace, so it runs beside searches and beside other calls.  The two kinds below add their buffers.
struct JoinWorkspace {
    hipStream_t stream = nullptr;
    // [0], [1]: around the step the host is about to wait for (timed); [2], [3]: around the clusters walk's rescore, which
    // is read one synchronise later than the join's
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // a pairs call: [0] candidates counted by the filter, [1] (low word) records written by the refine; a clusters call:
    // [0] ambiguous pairs of the launch, [1] its skipped tile pairs, [2] classes, [3] members
    uint64_t* d_counters = nullptr;
    uint64_t* h_counters = nullptr;  // pinned: where the host reads them

    int32_t init() {
        CS_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (hipEvent_t& e : ev) CS_HIP(hipEventCreate(&e));
        CS_HIP(realloc_buf(d_counters, 4));
        CS_HIP(realloc_buf(h_counters, 4, true));
        return CS_OK;
    }
    // counters [first, first + n) to the host, enqueued on the stream
    int32_t read_counters(uint32_t first, uint32_t n) {
        CS_HIP(hipMemcpyAsync(h_counters + first, d_counters + first, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        return CS_OK;
    }
    ~JoinWorkspace() {
        free_bufs(false, d_counters);
        free_bufs(true, h_counters);
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// A similar-pairs call's (scan_pairs.hip): the candidates and the qualifying records.
struct PairsWorkspace : JoinWorkspace {
    uint64_t* d_cand = nullptr; size_t cand_cap = 0;      // candidate pairs (rowA | rowB << 32)
    PairRecord* d_out = nullptr; size_t out_cap = 0;      // qualifying records

    ~PairsWorkspace() { free_bufs(false, d_cand, d_out); }
};

// A similar-clusters call's (scan_clusters.hip): O(stored rows) for the union-find and the labels, one word per tile, and
// the ambiguous buffer, whose size is fixed.
struct ClustersWorkspace : JoinWorkspace {
    uint32_t* d_parent = nullptr; size_t parent_cap = 0;        // [stored rows]
    uint32_t* d_mark = nullptr; size_t mark_cap = 0;            // [stored rows]: the label kernel's "this root was counted"
    uint32_t* d_tile_root = nullptr; size_t tile_root_cap = 0;  // [tiles]
    uint32_t* d_label = nullptr; size_t label_cap = 0;          // [ids issued]; a scoped call: ids, then labels, per list entry
    uint64_t* d_amb = nullptr; size_t amb_cap = 0;              // ambiguous pairs (rowA | rowB << 32)

    // (the ambiguous buffer is reserved beside the walk: a call without a join holds none)
    int32_t reserve(uint64_t stored, uint64_t tiles, uint64_t labels) {
        CS_TRY(reserve_buf(d_parent, parent_cap, (size_t)stored));
        CS_TRY(reserve_buf(d_mark, mark_cap, (size_t)stored));
        CS_TRY(reserve_buf(d_tile_root, tile_root_cap, (size_t)tiles));
        return reserve_buf(d_label, label_cap, (size_t)labels);
    }
    ~ClustersWorkspace() { free_bufs(false, d_parent, d_mark, d_tile_root, d_label, d_amb); }
};

void free_join_pools(cs_index* h) {
    for (PairsWorkspace* w : h->pairs_pool) delete w;
    for (ClustersWorkspace* w : h->clusters_pool) delete w;
}

}  // namespace cs

using namespace cs;

namespace {

constexpr const char* kPairs = "similar pairs";        // the calls' names in their messages
constexpr const char* kClusters = "similar clusters";

// What a call holds while it runs, given back when it returns on any path: a workspace of `pool` (h->pairs_pool,
// h->clusters_pool), and up to two f16 buffers of the call's own — the filter operand where the index's copy does not
// serve.  Such a buffer is freed here and never published through the handle, where a search running beside this call
// could pick the copy up just before it is freed.
template <class W>
struct JoinLease {
    cs_index* h;
    std::vector<W*>& pool;
    W* w = nullptr;
    _Float16* d_f16[2] = {nullptr, nullptr};

    ~JoinLease() {
        for (_Float16* p : d_f16)
            if (p) (void)hipFree(p);
        if (w) {
            std::lock_guard<std::mutex> lk(h->mu);
            pool.push_back(w);
        }
    }

    // a workspace from the pool, or a new one
    int32_t acquire(const char* what) {
        {
            std::lock_guard<std::mutex> lk(h->mu);
            if (!pool.empty()) {
                w = pool.back();
                pool.pop_back();
                return CS_OK;
            }
        }
        w = new W();
        if (w->init() == CS_OK) return CS_OK;
        delete w;
        w = nullptr;
        return fail(CS_ERR_HIP, "%s: could not create a HIP stream", what);
    }

    // d_f16[side]: `bytes` bytes (CS_FAULT_F16_ALLOC, tests: the allocation reports a failure)
    int32_t alloc_f16(const char* what, int side, size_t bytes) {
        if (cs_lab_env("CS_FAULT_F16_ALLOC") != nullptr || hipMalloc(&d_f16[side], bytes) != hipSuccess) {
            (void)hipGetLastError();
            d_f16[side] = nullptr;
            return fail(CS_ERR_OOM, "%s: no room for the f16 filter copy (%llu bytes)", what, (unsigned long long)bytes);
        }
        return CS_OK;
    }
};

// ---- the argument checks: each call sequences them itself, since the orders differ (the unscoped calls answer "fewer than
// two live rows" between check_join_dim and check_join_split; the scoped calls check their scopes before either)

// What every call checks first.  out_ok: none of the output buffers the call needs is null.
int32_t check_join(const cs_index* h, bool out_ok, int32_t mode, float min_cos) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    CS_TRY(check_search(h, 1, h->dim, 1));
    if (!out_ok) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (mode != CS_PAIRS_ALL && mode != CS_PAIRS_OTHER_GROUP)
        return fail(CS_ERR_BAD_ARG, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP (0..1), got %d", mode);
    if (min_cos != min_cos) return fail(CS_ERR_BAD_ARG, "min_cos is NaN");
    return CS_OK;
}

int32_t check_max_pairs(uint32_t max_pairs) {
    if (max_pairs == 0 || max_pairs > CS_MAX_PAIRS)
        return fail(CS_ERR_BAD_ARG, "max_pairs must be in 1..%u, got %u", CS_MAX_PAIRS, max_pairs);
    return CS_OK;
}

int32_t check_join_scopes(const cs_index* h, const cs_scope* scope_a, const cs_scope* scope_b) {
    if (!scope_a) return fail(CS_ERR_BAD_ARG, "null scope handle (scope_a)");
    if (!scope_b) return fail(CS_ERR_BAD_ARG, "null scope handle (scope_b)");
    CS_TRY(check_scope_handle(h, scope_a));
    return check_scope_handle(h, scope_b);
}

int32_t check_join_dim(const char* what, const cs_index* h) {
    if (!split_scan_supported(h->dim))
        return fail(CS_ERR_UNSUPPORTED, "%s need dim 384, 768 or 1024 (the f16 filter's widths), got %u", what, h->dim);
    return CS_OK;
}

int32_t check_join_split(const char* what, const cs_index* h) {
    if (!h->use_split) return fail(CS_ERR_UNSUPPORTED, "%s need the f16 filter copy, and CS_INDEX_SPLIT=0 turned it off", what);
    return CS_OK;
}

// ---- the steps the calls share

// The group table where the mode reads it, else the view of no table.
int32_t join_groups(cs_index* h, int32_t mode, GroupView* gv) {
    *gv = GroupView{nullptr, 0, h->ledger.id_base(), 0xFFFFFFFFu};
    return mode == CS_PAIRS_OTHER_GROUP ? ensure_groups(h, 0xFFFFFFFFu, gv) : CS_OK;
}

// The timed step of every call: `launch` (it enqueues on w->stream) between the workspace's first two events, `then` (what
// else the host is about to read: a read-back) behind them, ONE synchronise; ms grows by the time between the events.
template <class Launch, class Then>
int32_t timed(JoinWorkspace* w, double& ms, Launch&& launch, Then&& then) {
    CS_HIP(hipEventRecord(w->ev[0], w->stream));
    CS_TRY(launch());
    CS_HIP(hipEventRecord(w->ev[1], w->stream));
    CS_TRY(then());
    CS_HIP(hipStreamSynchronize(w->stream));
    float elapsed = 0.0f;
    CS_HIP(hipEventElapsedTime(&elapsed, w->ev[0], w->ev[1]));
    ms += elapsed;
    return CS_OK;
}

// The f16 rows a whole-store call filters on: *d_f16, `tiles` 128-row tiles.  The index's f16 copy where the index keeps one
// (the int8 copy does not serve it: ensure_f16, as a search would) or where an overflowed search left one (it stays until
// the next build).  Where the int8 copy serves, the index holds f32 + int8 and must go on doing so: the call converts the
// rows into a buffer of its OWN, the lease's (the same launch_corpus_split, the same tiles), on its workspace's stream —
// which is why the lease's workspace is acquired here, between the two.
template <class W>
int32_t whole_store_operand(const char* what, cs_index* h, JoinLease<W>& lease, uint64_t tiles, const _Float16** d_f16) {
    const uint64_t stored = h->ledger.stored();
    *d_f16 = nullptr;
    if (h->f16_eager || !q8_serves(h)) {
        if (!ensure_f16(h)) return fail(CS_ERR_OOM, "%s: no room for the f16 filter copy", what);
        *d_f16 = h->d_split;
    } else {
        std::lock_guard<std::mutex> lk(h->filter_mu);
        if (h->d_split && h->split_rows >= stored) *d_f16 = h->d_split;
    }
    CS_TRY(lease.acquire(what));
    if (*d_f16) return CS_OK;
    if (h->normed_rows < stored) return fail(CS_ERR_HIP, "%s: the index holds no row norms", what);
    CS_TRY(lease.alloc_f16(what, 0, (size_t)tiles * kPairsTileRows * h->dim * sizeof(_Float16)));
    CS_TRY(launch_corpus_split(h->d_corpus, h->d_norms, lease.d_f16[0], 0, stored, h->dim, lease.w->stream));
    *d_f16 = lease.d_f16[0];
    return CS_OK;
}

// Both lists of a scoped call refreshed, one after the other (no two scope mutexes are held together); the same handle
// twice is one list.
int32_t scopes_ready(cs_index* h, cs_scope* scope_a, cs_scope* scope_b, uint64_t* live_a, uint64_t* live_b) {
    CS_TRY(scope_ready(h, scope_a, live_a));
    if (scope_a == scope_b) *live_b = *live_a;
    else CS_TRY(scope_ready(h, scope_b, live_b));
    return CS_OK;
}

// The operand of a scoped call (PairsScopedPlan, ClustersScopedPlan): each side's rows packed into an f16 buffer of the
// call's own — lease.d_f16[0] and [1]; the same handle twice: [0] alone (scan_pairs_scoped.hip) — the index's d_split is
// neither read nor made.  First the one empty join the plan cannot see: two handles, one row each, the same row is no
// pair — plan.tile_pairs becomes 0 then, and where it is 0 nothing is allocated or packed (and lease.w may be null).
template <class W, class Plan>
int32_t pack_scopes(const char* what, cs_index* h, JoinLease<W>& lease, Plan& plan, const cs_scope* sa, const cs_scope* sb,
                    double& pack_ms) {
    W* const w = lease.w;
    const bool same = plan.triangle;
    if (plan.tile_pairs && !same && plan.rows_a == 1 && plan.rows_b == 1) {
        uint32_t* rows = reinterpret_cast<uint32_t*>(w->h_counters);
        CS_HIP(hipMemcpyAsync(rows, sa->d_list, sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        CS_HIP(hipMemcpyAsync(rows + 1, sb->d_list, sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        CS_HIP(hipStreamSynchronize(w->stream));
        if (rows[0] == rows[1]) plan.tile_pairs = 0;
    }
    if (plan.tile_pairs == 0) return CS_OK;
    if (h->normed_rows < h->ledger.stored()) return fail(CS_ERR_HIP, "%s: the index holds no row norms", what);
    CS_TRY(lease.alloc_f16(what, 0, packed_bytes_of(plan.tiles_a, h->dim)));
    if (!same) CS_TRY(lease.alloc_f16(what, 1, packed_bytes_of(plan.tiles_b, h->dim)));
    return timed(w, pack_ms, [&]() -> int32_t {
        CS_TRY(launch_pairs_pack(h->d_corpus, h->d_norms, sa->d_list, plan.rows_a, h->dim, lease.d_f16[0], w->stream));
        return same ? CS_OK : launch_pairs_pack(h->d_corpus, h->d_norms, sb->d_list, plan.rows_b, h->dim, lease.d_f16[1], w->stream);
    }, [] { return CS_OK; });
}

// ---- the similar-pairs search (scan_pairs.hip, plan: pairs_plan.hpp) -------------------------------------------
// What the calling thread's last successful call did (cs_index_similar_pairs_info).
struct PairsInfo {
    uint64_t candidates = 0;
    uint32_t bands = 0;
    double filter_ms = 0.0, refine_ms = 0.0, order_ms = 0.0;
    // a scoped call only (cs_index_similar_pairs_scoped_info; zeros after an unscoped one)
    double pack_ms = 0.0;
    uint64_t rows_a = 0, rows_b = 0, tile_pairs = 0;
};
thread_local PairsInfo last_pairs_info;

// The refusal of a call whose candidates outgrew its buffer, noticed after band `band` of `bands`.
int32_t pairs_overflow(uint64_t reached, uint64_t band, uint64_t bands, uint64_t cand_cap) {
    return fail(CS_ERR_UNSUPPORTED,
                "similar pairs: %llu candidate pairs after band %llu of %llu, more than the %llu this call holds "
                "(2 * max_pairs + 4096): raise min_cos, exclude groups (CS_PAIRS_OTHER_GROUP) or raise max_pairs",
                (unsigned long long)reached, (unsigned long long)band, (unsigned long long)bands, (unsigned long long)cand_cap);
}

// The bands of both pairs calls over `plan` (PairsPlan, PairsScopedPlan: bands, band, cand_cap): per band `launch(band)` —
// the filter, enqueued on w->stream — and one synchronise: the host reads the candidate counter and stops at the first
// overflow.
template <class Plan, class Launch>
int32_t pairs_bands(PairsWorkspace* w, const Plan& plan, PairsInfo& info, Launch&& launch) {
    for (uint64_t b = 0; b < plan.bands; ++b) {
        const PairsBand band = plan.band(b);
        CS_TRY(timed(w, info.filter_ms, [&] { return launch(band); }, [&] { return w->read_counters(0, 1); }));
        info.bands++;
        if (w->h_counters[0] > plan.cand_cap) return pairs_overflow(w->h_counters[0], b + 1, plan.bands, plan.cand_cap);
    }
    return CS_OK;
}

// The tail of both pairs calls, behind the last filter band (w->h_counters[0] = the candidates, within the buffer): the
// refine, the records' read-back and the ordering on the host into the caller's buffers; `info` becomes the thread's last.
int32_t pairs_finish(cs_index* h, PairsWorkspace* w, float min_cos, uint32_t max_pairs, uint32_t* out_a, uint32_t* out_b,
                     float* out_cos, uint64_t* out_total, PairsInfo& info) {
    const uint32_t ncand = (uint32_t)w->h_counters[0];
    info.candidates = ncand;
    std::vector<PairRecord> rec;
    if (ncand) {
        CS_TRY(timed(w, info.refine_ms, [&] {
            return launch_pairs_rescore(h->d_corpus, h->dim, w->d_cand, ncand, h->row_ids(), min_cos, w->d_out,
                                        reinterpret_cast<uint32_t*>(w->d_counters + 1), pairs_refine_blocks(ncand, h->num_cus),
                                        w->stream);
        }, [&] { return w->read_counters(1, 1); }));
        rec.resize((size_t)(uint32_t)w->h_counters[1]);
        if (!rec.empty()) {
            CS_HIP(hipMemcpyAsync(rec.data(), w->d_out, rec.size() * sizeof(PairRecord), hipMemcpyDeviceToHost, w->stream));
            CS_HIP(hipStreamSynchronize(w->stream));
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    const size_t keep = std::min<size_t>(rec.size(), max_pairs);
    std::partial_sort(rec.begin(), rec.begin() + keep, rec.end(), [](const PairRecord& x, const PairRecord& y) {
        if (x.cos != y.cos) return x.cos > y.cos;
        if (x.a != y.a) return x.a < y.a;
        return x.b < y.b;
    });
    for (size_t i = 0; i < keep; ++i) { out_a[i] = rec[i].a; out_b[i] = rec[i].b; out_cos[i] = rec[i].cos; }
    *out_total = rec.size();
    info.order_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    last_pairs_info = info;
    return CS_OK;
}

// ---- the similar-clusters search (scan_clusters.hip, plan: clusters_plan.hpp) -----------------------------------
// What the calling thread's last successful call did (cs_index_similar_clusters_info).
struct ClustersInfo {
    uint64_t scored = 0, skipped = 0, rescored = 0;
    uint32_t launches = 0;
    double join_ms = 0.0, label_ms = 0.0;
    // a scoped call only (cs_index_similar_clusters_scoped_info; zeros after an unscoped one)
    double pack_ms = 0.0;
    uint64_t rows_a = 0, rows_b = 0, vertices = 0;
};
thread_local ClustersInfo last_clusters_info;

// What every path of a clusters call ends in: the two counts where the caller wants them, `info` the thread's last.
int32_t clusters_answer(uint64_t* out_clusters, uint64_t* out_members, uint64_t clusters, uint64_t members, const ClustersInfo& info) {
    if (out_clusters) *out_clusters = clusters;
    if (out_members) *out_members = members;
    last_clusters_info = info;
    return CS_OK;
}

uint64_t clusters_knob(const char* name) {
    const char* e = cs_lab_env(name);  // (read per call: tests set it mid-process)
    return e ? std::strtoull(e, nullptr, 10) : 0;
}

// The time of the walk's last rescore, where one is still to be read (*pending): the caller has synchronised behind it.
int32_t rescore_time(ClustersWorkspace* w, bool& pending, ClustersInfo& info) {
    if (!pending) return CS_OK;
    float ms = 0.0f;
    CS_HIP(hipEventElapsedTime(&ms, w->ev[2], w->ev[3]));
    info.join_ms += ms;
    pending = false;
    return CS_OK;
}

// The device half of both clusters calls' walk (the decisions are ClustersWalk's, clusters_plan.hpp): per launch
// `roots_and_join(range)` — the tile roots and the join, enqueued on w->stream — and one synchronise to read the ambiguous
// counter — within the buffer: the rescore unites what qualifies; past it: the launch is void and its two halves are walked
// instead.  rescore_timed says that the last rescore's time is still to be read, behind the caller's next synchronise.
template <typename Plan, typename RootsAndJoin>
int32_t clusters_walk(cs_index* h, ClustersWorkspace* w, const Plan& plan, RowIds ids, float min_cos, ClustersInfo& info,
                      bool& rescore_timed, RootsAndJoin&& roots_and_join) {
    ClustersWalk<Plan> walk(plan);
    PairsBand r;
    rescore_timed = false;
    while (walk.next(r)) {
        CS_HIP(hipMemsetAsync(w->d_counters, 0, 2 * sizeof(uint64_t), w->stream));
        CS_TRY(timed(w, info.join_ms, [&] { return roots_and_join(r); }, [&] { return w->read_counters(0, 2); }));
        CS_TRY(rescore_time(w, rescore_timed, info));  // the previous launch's rescore has finished with this synchronise
        info.launches++;
        const uint64_t ambiguous = w->h_counters[0];
        const ClustersStep step = walk.report(r, ambiguous);
        if (step == ClustersStep::Impossible)
            return fail(CS_ERR_HIP, "similar clusters: one tile pair reported %llu ambiguous pairs, more than 128 * 128",
                        (unsigned long long)ambiguous);
        if (step == ClustersStep::Split) continue;
        info.skipped += w->h_counters[1];
        info.scored += r.count - w->h_counters[1];
        info.rescored += ambiguous;
        if (ambiguous) {
            CS_HIP(hipEventRecord(w->ev[2], w->stream));
            CS_TRY(launch_clusters_rescore(h->d_corpus, h->dim, w->d_amb, (uint32_t)ambiguous, ids, min_cos, w->d_parent,
                                           pairs_refine_blocks(ambiguous, h->num_cus), w->stream));
            CS_HIP(hipEventRecord(w->ev[3], w->stream));
            rescore_timed = true;
        }
    }
    return CS_OK;
}

// The tail of both clusters calls, behind the walk: `label` (the label pass, enqueued on w->stream: it leaves the labels in
// w->d_label and classes and members in counters [2] and [3]), the read-back of the two counters with `staged`, the first
// staged.size() words of w->d_label, and the late rescore time.  Labels are staged on the host and copied out by the caller
// last: a HIP failure half-way writes nothing either.
template <class Label>
int32_t clusters_finish(ClustersWorkspace* w, std::vector<uint32_t>& staged, bool rescore_timed, ClustersInfo& info,
                        Label&& label) {
    CS_TRY(timed(w, info.label_ms, label, [&]() -> int32_t {
        CS_TRY(w->read_counters(2, 2));
        CS_HIP(hipMemcpyAsync(staged.data(), w->d_label, staged.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, w->stream));
        return CS_OK;
    }));
    return rescore_time(w, rescore_timed, info);
}

}  // namespace

extern "C" {

// The checks, the plan, the f16 operand (whole_store_operand), the bands, the refine, the ordering on the host —
// std::partial_sort of the qualifying records only, by the total order (cosine desc, a asc, b asc), so the answer does not
// depend on how the device's atomics landed.
int32_t cs_index_similar_pairs(cs_index* h, float min_cos, int32_t mode, uint32_t max_pairs, uint32_t* out_a, uint32_t* out_b,
                               float* out_cos, uint64_t* out_total) {
    CS_TRY(check_join(h, out_a && out_b && out_cos && out_total, mode, min_cos));
    CS_TRY(check_max_pairs(max_pairs));
    CS_TRY(check_join_dim(kPairs, h));
    if (h->ledger.live() < 2) {  // no pair: nothing is launched
        *out_total = 0;
        last_pairs_info = PairsInfo{};
        return CS_OK;
    }
    CS_TRY(check_join_split(kPairs, h));
    DeviceGuard g(h->device);
    const uint64_t stored = h->ledger.stored();
    const PairsPlan plan = plan_pairs(stored, max_pairs, h->num_cus);
    JoinLease<PairsWorkspace> lease{h, h->pairs_pool};
    const _Float16* d_f16 = nullptr;
    CS_TRY(whole_store_operand(kPairs, h, lease, plan.tiles, &d_f16));
    PairsWorkspace* w = lease.w;
    GroupView gv;
    CS_TRY(join_groups(h, mode, &gv));
    CS_TRY(reserve_buf(w->d_cand, w->cand_cap, (size_t)plan.cand_cap));
    CS_TRY(reserve_buf(w->d_out, w->out_cap, (size_t)plan.cand_cap));
    CS_HIP(hipMemsetAsync(w->d_counters, 0, 2 * sizeof(uint64_t), w->stream));
    const uint32_t* d_dead = h->ledger.removed() ? h->d_dead : nullptr;
    PairsInfo info;
    CS_TRY(pairs_bands(w, plan, info, [&](const PairsBand& band) {
        return launch_pairs_filter(d_f16, h->dim, plan.tiles, band.first, band.count, stored, d_dead, h->row_ids(), gv,
                                   mode == CS_PAIRS_OTHER_GROUP, min_cos, h->filter_margin, w->d_cand, w->d_counters,
                                   (uint32_t)plan.cand_cap, w->stream);
    }));
    return pairs_finish(h, w, min_cos, max_pairs, out_a, out_b, out_cos, out_total, info);
}

// cs_index_similar_pairs over the row lists of two scopes (the same handle twice: inside one).  Every
// check comes before a list is refreshed; then each side's rows are packed (pack_scopes), the plan's triangle or rectangle
// is filtered in bands, and the tail is the unscoped call's (pairs_finish).  A join the plan says is empty acquires
// nothing.  The scopes' route counters do not move: this is no search.
int32_t cs_index_similar_pairs_scoped(cs_index* h, cs_scope* scope_a, cs_scope* scope_b, float min_cos, int32_t mode,
                                      uint32_t max_pairs, uint32_t* out_a, uint32_t* out_b, float* out_cos, uint64_t* out_total) {
    CS_TRY(check_join(h, out_a && out_b && out_cos && out_total, mode, min_cos));
    CS_TRY(check_max_pairs(max_pairs));
    CS_TRY(check_join_scopes(h, scope_a, scope_b));
    CS_TRY(check_join_dim(kPairs, h));
    CS_TRY(check_join_split(kPairs, h));
    DeviceGuard g(h->device);
    uint64_t live_a = 0, live_b = 0;
    CS_TRY(scopes_ready(h, scope_a, scope_b, &live_a, &live_b));
    PairsScopedPlan plan = plan_pairs_scoped(scope_a == scope_b, live_a, live_b, max_pairs);
    cs_scope* const sa = plan.swapped ? scope_b : scope_a;
    cs_scope* const sb = plan.swapped ? scope_a : scope_b;
    PairsInfo info;
    info.rows_a = plan.rows_a;
    info.rows_b = plan.rows_b;
    JoinLease<PairsWorkspace> lease{h, h->pairs_pool};
    if (plan.tile_pairs) {
        CS_TRY(lease.acquire(kPairs));
        CS_TRY(reserve_buf(lease.w->d_cand, lease.w->cand_cap, (size_t)plan.cand_cap));
        CS_TRY(reserve_buf(lease.w->d_out, lease.w->out_cap, (size_t)plan.cand_cap));
        CS_HIP(hipMemsetAsync(lease.w->d_counters, 0, 2 * sizeof(uint64_t), lease.w->stream));
    }
    CS_TRY(pack_scopes(kPairs, h, lease, plan, sa, sb, info.pack_ms));
    if (plan.tile_pairs == 0) {  // no pair: no filter is launched
        *out_total = 0;
        last_pairs_info = info;
        return CS_OK;
    }
    info.tile_pairs = plan.tile_pairs;
    PairsWorkspace* w = lease.w;
    GroupView gv;
    CS_TRY(join_groups(h, mode, &gv));
    const _Float16* d_b = plan.triangle ? lease.d_f16[0] : lease.d_f16[1];
    CS_TRY(pairs_bands(w, plan, info, [&](const PairsBand& band) {
        return launch_pairs_scoped_filter(plan, lease.d_f16[0], d_b, sa->d_list, sb->d_list, h->dim, band.first, band.count,
                                          h->row_ids(), gv, mode == CS_PAIRS_OTHER_GROUP, min_cos, h->filter_margin, w->d_cand,
                                          w->d_counters, w->stream);
    }));
    return pairs_finish(h, w, min_cos, max_pairs, out_a, out_b, out_cos, out_total, info);
}

// The checks; the f16 operand as cs_index_similar_pairs finds or makes it; then the plan's walk (clusters_walk) and at the end the
// label kernel (clusters_finish).
int32_t cs_index_similar_clusters(cs_index* h, float min_cos, int32_t mode, uint32_t* out_label, uint64_t n_labels,
                                  uint64_t* out_clusters, uint64_t* out_members) {
    CS_TRY(check_join(h, out_label != nullptr, mode, min_cos));
    const uint64_t issued = h->ledger.issued_ids();
    if (n_labels != issued)
        return fail(CS_ERR_BAD_ARG, "n_labels must be cs_index_next_id - id_base = %llu (one label per id issued), got %llu",
                    (unsigned long long)issued, (unsigned long long)n_labels);
    CS_TRY(check_join_dim(kClusters, h));
    const uint64_t stored = h->ledger.stored();
    if (h->ledger.live() < 2) {  // no pair: every live id is its own label, nothing is launched
        std::vector<uint32_t> rows;
        h->ledger.survivors(0, stored, rows);
        std::fill(out_label, out_label + n_labels, (uint32_t)CS_NO_ID);
        for (uint32_t r : rows) {
            const uint32_t id = h->ledger.compacted() ? h->ledger.ids_data()[r] : h->ledger.id_base() + r;
            out_label[id - h->ledger.id_base()] = id;
        }
        return clusters_answer(out_clusters, out_members, 0, 0, ClustersInfo{});
    }
    CS_TRY(check_join_split(kClusters, h));
    DeviceGuard g(h->device);
    const ClustersPlan plan = plan_clusters(stored, clusters_knob("CS_CLUSTERS_LAUNCH_TILE_PAIRS"),
                                            clusters_knob("CS_CLUSTERS_AMBIGUOUS_CAP"));
    JoinLease<ClustersWorkspace> lease{h, h->clusters_pool};
    const _Float16* d_f16 = nullptr;
    CS_TRY(whole_store_operand(kClusters, h, lease, plan.tiles, &d_f16));
    ClustersWorkspace* w = lease.w;
    GroupView gv;
    CS_TRY(join_groups(h, mode, &gv));
    CS_TRY(w->reserve(stored, plan.tiles, n_labels));
    CS_TRY(reserve_buf(w->d_amb, w->amb_cap, (size_t)plan.ambiguous_cap));
    CS_HIP(hipMemsetAsync(w->d_counters, 0, 4 * sizeof(uint64_t), w->stream));
    CS_HIP(hipMemsetAsync(w->d_label, 0xFF, (size_t)n_labels * sizeof(uint32_t), w->stream));  // CS_NO_ID
    CS_TRY(launch_clusters_init(w->d_parent, w->d_mark, stored, w->stream));
    const uint32_t* d_dead = h->ledger.removed() ? h->d_dead : nullptr;
    const float* d_norms = h->normed_rows >= stored ? h->d_norms : nullptr;  // none: no pair is united without a rescore
    const RowIds ids = h->row_ids();
    ClustersInfo info;
    bool rescore_timed = false;
    CS_TRY(clusters_walk(h, w, plan, ids, min_cos, info, rescore_timed, [&](const PairsBand& r) -> int32_t {
        CS_TRY(launch_clusters_tile_roots(w->d_parent, plan.tiles, stored, d_dead, w->d_tile_root, w->stream));
        return launch_clusters_join(d_f16, h->dim, plan.tiles, r.first, r.count, stored, d_dead, ids, gv,
                                    mode == CS_PAIRS_OTHER_GROUP, min_cos, h->filter_margin, d_norms, w->d_parent,
                                    w->d_tile_root, w->d_amb, w->d_counters, (uint32_t)plan.ambiguous_cap, w->stream);
    }));
    std::vector<uint32_t> staged((size_t)n_labels);
    CS_TRY(clusters_finish(w, staged, rescore_timed, info, [&] {
        return launch_clusters_label(w->d_parent, w->d_mark, stored, d_dead, ids, w->d_label, n_labels, w->d_counters + 2, w->stream);
    }));
    std::copy(staged.begin(), staged.end(), out_label);
    return clusters_answer(out_clusters, out_members, w->h_counters[2], w->h_counters[3], info);
}

// cs_index_similar_clusters over the graph of cs_index_similar_pairs_scoped (scan_clusters_scoped.hip, plan:
// clusters_scoped_plan.hpp).  Every check comes before a list is refreshed; the lists are refreshed and packed as
// that call does, and the walk is cs_index_similar_clusters'.  The union-find is the pooled workspace's, sized by stored
// rows, but only the words of the scopes' rows are initialised and reached: the device work of a call is O(live rows of the
// scopes).  The label pass writes (id, label) per list entry; the host interleaves the two ascending segments, dropping the
// second copy of a row in both, and copies out last.  An empty join (the plan's tile_pairs == 0, or two handles holding the
// same single row) runs the init and the label pass only.
int32_t cs_index_similar_clusters_scoped(cs_index* h, cs_scope* scope_a, cs_scope* scope_b, float min_cos, int32_t mode,
                                         uint32_t* out_ids, uint32_t* out_label, uint64_t cap, uint64_t* out_n,
                                         uint64_t* out_clusters, uint64_t* out_members) {
    CS_TRY(check_join(h, out_ids && out_label && out_n, mode, min_cos));
    CS_TRY(check_join_scopes(h, scope_a, scope_b));
    const bool same = scope_a == scope_b;
    const uint64_t want = scope_a->n_ids + (same ? 0 : scope_b->n_ids);  // (n_ids never changes after the create call)
    if (cap < want)
        return fail(CS_ERR_BAD_ARG, "cap must be at least n_ids(scope_a)%s = %llu (one slot per id a scope names), got %llu",
                    same ? "" : " + n_ids(scope_b)", (unsigned long long)want, (unsigned long long)cap);
    CS_TRY(check_join_dim(kClusters, h));
    CS_TRY(check_join_split(kClusters, h));
    DeviceGuard g(h->device);
    uint64_t live_a = 0, live_b = 0;
    CS_TRY(scopes_ready(h, scope_a, scope_b, &live_a, &live_b));
    ClustersScopedPlan plan = plan_clusters_scoped(same, live_a, live_b, clusters_knob("CS_CLUSTERS_LAUNCH_TILE_PAIRS"),
                                                   clusters_knob("CS_CLUSTERS_AMBIGUOUS_CAP"));
    cs_scope* const sa = plan.swapped ? scope_b : scope_a;
    cs_scope* const sb = plan.swapped ? scope_a : scope_b;
    const uint64_t second = same ? 0 : plan.rows_b;   // entries of the B segment of the label pass
    const uint64_t entries = plan.rows_a + second;
    ClustersInfo info;
    info.rows_a = plan.rows_a;
    info.rows_b = plan.rows_b;
    if (entries == 0) {  // no vertex
        *out_n = 0;
        return clusters_answer(out_clusters, out_members, 0, 0, info);
    }
    JoinLease<ClustersWorkspace> lease{h, h->clusters_pool};
    CS_TRY(lease.acquire(kClusters));
    ClustersWorkspace* w = lease.w;
    CS_TRY(w->reserve(h->ledger.stored(), plan.tiles_a + plan.tiles_b, 2 * entries));  // labels: ids, then labels, per list entry
    CS_HIP(hipMemsetAsync(w->d_counters, 0, 4 * sizeof(uint64_t), w->stream));
    CS_TRY(launch_clusters_scoped_init(w->d_parent, w->d_mark, sa->d_list, plan.rows_a, sb->d_list, second, w->stream));
    CS_TRY(pack_scopes(kClusters, h, lease, plan, sa, sb, info.pack_ms));
    const RowIds ids = h->row_ids();
    bool rescore_timed = false;
    if (plan.tile_pairs) {
        GroupView gv;
        CS_TRY(join_groups(h, mode, &gv));
        CS_TRY(reserve_buf(w->d_amb, w->amb_cap, (size_t)plan.ambiguous_cap));
        const _Float16* d_b = same ? lease.d_f16[0] : lease.d_f16[1];
        uint32_t* const d_root_a = w->d_tile_root;
        uint32_t* const d_root_b = same ? d_root_a : d_root_a + plan.tiles_a;
        CS_TRY(clusters_walk(h, w, plan, ids, min_cos, info, rescore_timed, [&](const PairsBand& r) -> int32_t {
            CS_TRY(launch_clusters_scoped_tile_roots(w->d_parent, sa->d_list, plan.rows_a, d_root_a, w->stream));
            if (!same) CS_TRY(launch_clusters_scoped_tile_roots(w->d_parent, sb->d_list, plan.rows_b, d_root_b, w->stream));
            return launch_clusters_scoped_join(plan, lease.d_f16[0], d_b, sa->d_list, sb->d_list, h->dim, r.first, r.count, ids, gv,
                                               mode == CS_PAIRS_OTHER_GROUP, min_cos, h->filter_margin, h->d_norms, w->d_parent,
                                               d_root_a, d_root_b, w->d_amb, w->d_counters, w->stream);
        }));
    }
    std::vector<uint32_t> staged((size_t)(2 * entries));
    CS_TRY(clusters_finish(w, staged, rescore_timed, info, [&] {
        return launch_clusters_scoped_label(w->d_parent, w->d_mark, sa->d_list, plan.rows_a, sb->d_list, second, ids, w->d_label,
                                            w->d_label + entries, w->d_counters + 2, w->stream);
    }));
    // the two segments ascend by id (rows ascend with ids): one merge, a row of both lists once.  At most `entries` <= cap.
    const uint32_t* const sid = staged.data();
    const uint32_t* const slab = staged.data() + entries;
    uint64_t n = 0, i = 0, j = plan.rows_a;
    while (i < plan.rows_a || j < entries) {
        uint64_t take;
        if (j >= entries || (i < plan.rows_a && sid[i] <= sid[j])) {
            if (j < entries && sid[i] == sid[j]) ++j;
            take = i++;
        } else {
            take = j++;
        }
        out_ids[n] = sid[take];
        out_label[n] = slab[take];
        ++n;
    }
    *out_n = n;
    info.vertices = n;
    return clusters_answer(out_clusters, out_members, w->h_counters[2], w->h_counters[3], info);
}

int32_t cs_index_similar_clusters_info(uint64_t* tile_pairs_scored, uint64_t* tile_pairs_skipped, uint64_t* rescored_pairs,
                                       uint32_t* launches, double* join_ms, double* label_ms) {
    const ClustersInfo& i = last_clusters_info;
    if (tile_pairs_scored) *tile_pairs_scored = i.scored;
    if (tile_pairs_skipped) *tile_pairs_skipped = i.skipped;
    if (rescored_pairs) *rescored_pairs = i.rescored;
    if (launches) *launches = i.launches;
    if (join_ms) *join_ms = i.join_ms;
    if (label_ms) *label_ms = i.label_ms;
    return CS_OK;
}

int32_t cs_index_similar_clusters_scoped_info(double* pack_ms, uint64_t* rows_a, uint64_t* rows_b, uint64_t* vertices) {
    const ClustersInfo& i = last_clusters_info;
    if (pack_ms) *pack_ms = i.pack_ms;
    if (rows_a) *rows_a = i.rows_a;
    if (rows_b) *rows_b = i.rows_b;
    if (vertices) *vertices = i.vertices;
    return CS_OK;
}

int32_t cs_index_similar_pairs_scoped_info(double* pack_ms, uint64_t* rows_a, uint64_t* rows_b, uint64_t* tile_pairs) {
    const PairsInfo& i = last_pairs_info;
    if (pack_ms) *pack_ms = i.pack_ms;
    if (rows_a) *rows_a = i.rows_a;
    if (rows_b) *rows_b = i.rows_b;
    if (tile_pairs) *tile_pairs = i.tile_pairs;
    return CS_OK;
}

int32_t cs_index_similar_pairs_info(uint64_t* candidates, uint32_t* bands, double* filter_ms, double* refine_ms, double* order_ms) {
    const PairsInfo& i = last_pairs_info;
    if (candidates) *candidates = i.candidates;
    if (bands) *bands = i.bands;
    if (filter_ms) *filter_ms = i.filter_ms;
    if (refine_ms) *refine_ms = i.refine_ms;
    if (order_ms) *order_ms = i.order_ms;
    return CS_OK;
}

}  // extern "C"
