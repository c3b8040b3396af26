// index.hip — cs_index_*: the vector half of the reference's VectorStore
// (/root/reference/src/vectordb/store.rs:94-750) as a device-resident row-major matrix
// searched by the exact scan of scan.hip.  Metadata (store.rs:19-85) stays with the caller.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <utility>
#include <vector>

#include <cstdlib>

#include "grouped_plan.hpp"
#include "index_internal.hpp"
#include "masked_plan.hpp"
#include "scope_ops_plan.hpp"
#include "similar_route.hpp"
#include "similar_sources.hpp"

namespace cs {

std::string& last_error_ref() {
    static thread_local std::string msg;
    return msg;
}

int32_t fail(int32_t code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return code;
}

// Per-call scratch.  Host-API calls borrow one from the pool (own stream); device-API
// calls use the one bound to the caller's stream (stream order makes reuse safe).
struct Workspace {
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t* d_partial = nullptr; size_t partial_cap = 0;
    uint64_t* d_tmp_a = nullptr; uint64_t* d_tmp_b = nullptr; size_t tmp_a_cap = 0, tmp_b_cap = 0;
    ScanPrime prime; size_t wave_max_cap = 0, done_cap = 0, floor_cap = 0;
    float* d_queries = nullptr; size_t q_cap = 0;
    uint64_t* d_keys = nullptr; float* d_cos = nullptr; uint32_t* d_ids = nullptr; size_t keys_cap = 0, cos_cap = 0, ids_cap = 0;
    uint32_t* d_counts = nullptr; size_t counts_cap = 0;
    // pinned staging of the host-buffer API: queries in, packed keys out (ONE copy each way; the host
    // unpacks cosine / id / count from the keys — three more small D2H copies cost ~8 us apiece)
    float* h_queries = nullptr; size_t h_q_cap = 0;
    uint64_t* h_keys = nullptr; size_t h_keys_cap = 0;
    uint32_t* h_variant_meta = nullptr;  // pinned: [0] count, [1] high-confidence flag (cs_index_search_variants)
    // masked searches (run_masked): the words of the caller's mask that cover the index's ids, the row list and the
    // row-list pass's per-block offsets (+ the list length)
    uint32_t* d_allow = nullptr; uint32_t* d_list = nullptr; uint32_t* d_mblocks = nullptr;
    size_t allow_cap = 0, list_cap = 0, mblocks_cap = 0;
    // similar-chunk searches (search_similar): per query the source's stored row, its excluded id and its excluded group,
    // [3][nq] — resolved on the host into the pinned copy, one copy to the device
    uint32_t* h_similar = nullptr; uint32_t* d_similar = nullptr;
    size_t h_similar_cap = 0, d_similar_cap = 0;
    // boosted searches (search_boosted): the call's weight table — pinned, then one copy to the device — and the pinned
    // [nq][k] cosines of the winners, which the cosine pass writes beside the keys
    float* h_weights = nullptr; float* d_weights = nullptr; float* h_winner_cos = nullptr;
    size_t h_weights_cap = 0, d_weights_cap = 0, h_winner_cos_cap = 0;
    // boosted searches over query variants (search_variants_boosted): the [k] merged keys, between the variants merge and
    // the cosine pass
    uint64_t* d_merged = nullptr; size_t merged_cap = 0;
    std::vector<EventTriple> free_events;
    BatchedState bs;
    size_t cnt_cap = 0, tau_cap = 0, cand_cap = 0, carry_cap = 0;
    SplitQueryWs qw;
    size_t qsplit_cap = 0, qmag_cap = 0, qmeta_cap = 0, q8_elems = 0;
    uint32_t* h_overflow = nullptr;
    uint32_t mirror_seen = 0;  // value of h_overflow[3] already accounted for
    bool last_via_q8 = false;  // the previous filter search on this workspace read the int8 copy (strike bookkeeping)

    // want_q8: the int8 copy is this search's filter operand — its three query planes are allocated only then, and
    // *q8_ok = false (never an error) when they do not fit: the caller filters on the f16 copy instead
    int32_t reserve_split_queries(uint32_t nq, uint32_t dim, bool want_q8, bool* q8_ok) {
        const size_t elems = (size_t)nq * dim;
        CS_TRY(reserve_buf(qw.d_qsplit, qsplit_cap, elems));
        if (want_q8 && elems > q8_elems) {
            q8_elems = 0;
            qw.d_q8q_lo = nullptr;
            if (realloc_buf(qw.d_q8q, elems) == hipSuccess && realloc_buf(qw.d_q8q_hi, 2 * elems) == hipSuccess) {
                qw.d_q8q_lo = qw.d_q8q_hi + elems;
                q8_elems = elems;
            } else {
                (void)hipGetLastError();
                free_bufs(false, qw.d_q8q, qw.d_q8q_hi);
            }
        }
        *q8_ok = want_q8 && elems <= q8_elems;
        CS_TRY(reserve_buf(qw.d_qmag, qmag_cap, nq));
        return reserve_buf(qw.d_qmeta, qmeta_cap, 4 * (size_t)nq);
    }

    int32_t reserve_prime(const ScanPlan& pp, uint32_t nq) {
        CS_TRY(reserve_buf(prime.d_wave_max, wave_max_cap, (size_t)nq * pp.blocks * 4));
        if (nq > done_cap) {  // passes <= nq
            CS_TRY(reserve_buf(prime.d_done, done_cap, nq));
            CS_HIP(hipMemset(prime.d_done, 0, nq * sizeof(uint32_t)));
        }
        return reserve_buf(prime.d_floor, floor_cap, nq);
    }

    int32_t reserve_masked(uint64_t words, uint64_t list_rows, uint32_t list_blocks) {
        CS_TRY(reserve_buf(d_allow, allow_cap, words));
        CS_TRY(reserve_buf(d_list, list_cap, list_rows));
        return reserve_buf(d_mblocks, mblocks_cap, (size_t)list_blocks + 1);
    }

    int32_t reserve_similar(uint32_t nq) {
        CS_TRY(reserve_buf(h_similar, h_similar_cap, 3 * (size_t)nq, true));
        return reserve_buf(d_similar, d_similar_cap, 3 * (size_t)nq);
    }

    int32_t reserve_boosted(uint32_t nq, uint32_t k, uint32_t n_classes) {
        CS_TRY(reserve_buf(h_weights, h_weights_cap, n_classes, true));
        CS_TRY(reserve_buf(d_weights, d_weights_cap, n_classes));
        return reserve_buf(h_winner_cos, h_winner_cos_cap, (size_t)nq * k, true);
    }

    int32_t reserve_boosted_variants(uint32_t k, uint32_t n_classes) {
        CS_TRY(reserve_boosted(1, k, n_classes));
        return reserve_buf(d_merged, merged_cap, k);
    }

    int32_t reserve_batched(uint32_t nq, uint32_t k) {
        if (!h_overflow) {
            CS_HIP(realloc_buf(h_overflow, 4, true));
            h_overflow[3] = 0;
            bs.h_mirror = h_overflow + 3;  // written by the device (scan.hpp BatchedState::h_mirror)
        }
        if (!bs.d_overflow) {  // [0] this search, [1] sticky, [2] overflowed searches so far (scan.hpp BatchedState)
            CS_HIP(realloc_buf(bs.d_overflow, 4));
            CS_HIP(hipMemset(bs.d_overflow, 0, 4 * sizeof(uint32_t)));
        }
        CS_TRY(reserve_buf(bs.d_cnt, cnt_cap, (size_t)nq * kCntStride));
        CS_TRY(reserve_buf(bs.d_tau, tau_cap, nq));
        CS_TRY(reserve_buf(bs.d_cand, cand_cap, (size_t)nq * batched_cap(k)));
        return reserve_buf(bs.d_carry, carry_cap, (size_t)nq * k);
    }

    // partial_keys / merge_keys: the room the search kind's plan asks for (ScanPlan, GroupedPlan)
    int32_t reserve(size_t partial_keys, size_t merge_keys, uint32_t nq, uint32_t dim, uint32_t k, bool host_io) {
        CS_TRY(reserve_buf(d_partial, partial_cap, partial_keys));
        CS_TRY(reserve_buf(d_tmp_a, tmp_a_cap, merge_keys));
        CS_TRY(reserve_buf(d_tmp_b, tmp_b_cap, merge_keys));
        if (!host_io) return CS_OK;
        const size_t qn = (size_t)nq * dim, on = (size_t)nq * k;
        CS_TRY(reserve_buf(d_queries, q_cap, qn));
        CS_TRY(reserve_buf(d_keys, keys_cap, on));
        CS_TRY(reserve_buf(d_cos, cos_cap, on));
        CS_TRY(reserve_buf(d_ids, ids_cap, on));
        CS_TRY(reserve_buf(d_counts, counts_cap, nq));
        CS_TRY(reserve_buf(h_keys, h_keys_cap, on, true));
        return reserve_buf(h_queries, h_q_cap, qn, true);
    }

    // the overflow word of the search just enqueued (host-buffer API: it synchronises for its results anyway)
    int32_t read_overflow(hipStream_t s, bool* overflow) {
        CS_HIP(hipMemcpyAsync(h_overflow, bs.d_overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        CS_HIP(hipStreamSynchronize(s));
        *overflow = *h_overflow != 0;
        return CS_OK;
    }

    void release_all() {
        free_bufs(false, d_partial, d_tmp_a, d_tmp_b, d_queries, d_keys, d_cos, d_ids, d_counts, prime.d_wave_max, prime.d_done,
                  prime.d_floor, bs.d_cand, bs.d_cnt, bs.d_tau, bs.d_carry, bs.d_overflow, qw.d_qsplit, qw.d_qmag, qw.d_q8q,
                  qw.d_q8q_hi, qw.d_qmeta, d_allow, d_list, d_mblocks, d_similar, d_weights, d_merged);
        free_bufs(true, h_keys, h_queries, h_overflow, h_variant_meta, h_similar, h_weights, h_winner_cos);
        for (auto& t : free_events) {
            (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); (void)hipEventDestroy(t.e2);
        }
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

// ---- what index_joins.hip calls as well (index_internal.hpp); scope_ready is further down, beside the scopes

// the int8 copy is the filter's operand: it exists, was not retired, and reaches past phase 0's rows
bool q8_serves(const cs_index* h) {
    return h->use_q8 && h->d_q8 && h->d_tmeta && h->q8_active.load() && h->q8_rows > kFilterPhase0;
}

// The f16 copy, complete for the rows of the last build — built now if it is not there (allocation + one conversion pass
// over the missing rows on the null stream, waited for: 7.68 GB and ~4.7 ms per 10M x 384, paid once, by the first
// search that needs it).  false: no room (remembered until clear()).
bool ensure_f16(cs_index* h) {
    if (!h->use_split) return false;
    std::lock_guard<std::mutex> lk(h->filter_mu);
    if (h->d_split && h->split_rows >= h->ledger.stored()) return true;
    if (h->f16_failed || h->normed_rows < h->ledger.stored()) return false;
    const size_t cap256 = ((size_t)h->capacity + 255) / 256 * 256;
    if (!h->d_split || h->split_cap < cap256) {
        if (h->d_split) (void)hipFree(h->d_split);
        h->d_split = nullptr; h->split_rows = 0; h->split_cap = 0;
        if (cs_lab_env("CS_FAULT_F16_ALLOC") != nullptr || hipMalloc(&h->d_split, cap256 * h->dim * sizeof(_Float16)) != hipSuccess) {
            (void)hipGetLastError();
            h->d_split = nullptr;
            h->f16_failed = true;
            return false;
        }
        h->split_cap = cap256;
    }
    if (launch_corpus_split(h->d_corpus, h->d_norms, h->d_split, h->split_rows, h->ledger.stored() - h->split_rows, h->dim, nullptr) != CS_OK ||
        hipStreamSynchronize(nullptr) != hipSuccess) {
        (void)hipGetLastError();
        h->f16_failed = true;
        return false;
    }
    h->split_rows = h->ledger.stored();
    return true;
}

// The handle-level checks of a scoped search: they read nothing that a refresh writes and take no lock.
int32_t check_scope_handle(const cs_index* h, const cs_scope* sc) {
    if (!sc) return fail(CS_ERR_BAD_ARG, "null scope handle");
    if (sc->index != h) return fail(CS_ERR_BAD_ARG, "the scope was made for another store");
    return CS_OK;
}

// The group table as this search's kernels read it.  A dirty table is brought up to date first, under groups_mu, with
// synchronous copies (and after the device has finished what was enqueued, when the table has to move): a concurrent
// grouped search either waits here or finds it clean.  No group assigned: a null table, every id CS_NO_GROUP.
int32_t ensure_groups(cs_index* h, uint32_t per_group, GroupView* gv) {
    std::lock_guard<std::mutex> lk(h->groups_mu);
    *gv = GroupView{nullptr, 0, h->ledger.id_base(), per_group};
    if (h->groups.assigned() == 0) return CS_OK;
    const uint64_t n = h->groups.size();
    if (n > h->groups_cap) {
        CS_HIP(hipDeviceSynchronize());  // a search that was only enqueued may still read the old table
        const uint64_t cap = std::max<uint64_t>(n, std::min<uint64_t>(2 * h->groups_cap, 0xffffffffull));
        h->groups_cap = 0;
        h->groups.uploaded(0);  // the new table holds nothing yet
        CS_HIP(realloc_buf(h->d_groups, (size_t)cap));
        h->groups_cap = cap;
    }
    uint64_t lo = 0, hi = 0;
    if (h->groups.pending(&lo, &hi))
        CS_HIP(hipMemcpy(h->d_groups + lo, h->groups.data() + lo, (size_t)(hi - lo) * sizeof(uint32_t), hipMemcpyHostToDevice));
    h->groups.uploaded(n);
    gv->groups = h->d_groups;
    gv->len = (uint32_t)n;
    return CS_OK;
}

int32_t check_search(const cs_index* h, uint32_t nq, uint32_t dim, uint32_t k) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (dim != h->dim)  // store.rs:432-438
        return fail(CS_ERR_DIM_MISMATCH,
                    "Query embedding dimension mismatch: expected %u, got %u", h->dim, dim);
    if (!h->built)  // store.rs:440-444
        return fail(CS_ERR_NOT_BUILT,
                    "Index not built. Call build_index() after inserting chunks.");
    if (nq == 0 || nq > CS_MAX_QUERIES)
        return fail(CS_ERR_BAD_ARG, "nq must be in 1..%u, got %u", CS_MAX_QUERIES, nq);
    if (k == 0 || k > CS_MAX_K)
        return fail(CS_ERR_BAD_ARG, "k must be in 1..%u, got %u", CS_MAX_K, k);
    return CS_OK;
}

}  // namespace cs

using namespace cs;

namespace {

// Appends through cs_index_add_device / index_append_from may still be in flight on caller streams that do not
// order against the null stream (hipStreamNonBlocking, torch side streams) or that belong to another device.
int32_t drain_appends(cs_index* h) {
    int32_t st = CS_OK;
    for (const auto& fe : h->foreign_appends) {
        DeviceGuard g(fe.device);
        if (hipEventSynchronize(fe.done) != hipSuccess && st == CS_OK)
            st = fail(CS_ERR_HIP, "a peer append into the index did not complete: %s", hipGetErrorString(hipGetLastError()));
        (void)hipEventDestroy(fe.done);
    }
    h->foreign_appends.clear();
    // (the index's own device is drained whether or not a peer reported a failure)
    if (hipDeviceSynchronize() != hipSuccess && st == CS_OK)
        st = fail(CS_ERR_HIP, "hipDeviceSynchronize failed: %s", hipGetErrorString(hipGetLastError()));
    return st;
}

// New buffers of a grow(), freed on every path that does not commit them (a failing copy between the
// allocations and the pointer swap used to return with nc / nd / nn / n8 / nm still allocated).
struct GrowBuffers {
    float* nc = nullptr;      // corpus
    uint32_t* nd = nullptr;   // tombstone bitmap
    float* nn = nullptr;      // row norms
    _Float16* ns = nullptr;   // f16 filter copy
    int8_t* n8 = nullptr;     // int8 filter copy
    float4* nm = nullptr;     // its tile metadata
    ~GrowBuffers() {
        for (void* p : {(void*)nc, (void*)nd, (void*)nn, (void*)ns, (void*)n8, (void*)nm})
            if (p) (void)hipFree(p);
    }
};

// CS_FAULT_GROW_COPY=<stage> (tests): the copy of that stage reports a failure — 1 f16 copy, 2 int8 copy, 3 bitmap clear,
// 4 norms, 5 corpus, 6 bitmap upload
static bool grow_fault(int stage, const cs_index* h) {
    const char* e = cs_lab_env("CS_FAULT_GROW_COPY");  // (read per call: a grow is rare, and tests set it mid-process)
    return e && std::atoi(e) == stage && h->capacity != 0;
}
#define CS_GROW_COPY(stage, call)                                                                            \
    do {                                                                                                     \
        const hipError_t _e = grow_fault(stage, h) ? hipErrorUnknown : (call);                               \
        if (_e != hipSuccess)                                                                                \
            return fail(CS_ERR_HIP, "growing the index: copy stage %d failed: %s", stage, hipGetErrorString(_e)); \
    } while (0)

// Transactional: every new buffer is allocated and filled first; the handle's pointers are swapped (and the old buffers
// freed) only after the last copy succeeded.  A failure leaves the index exactly as it was and frees what was allocated.
// Two degradations are not failures: without room for a larger f16 / int8 filter copy that copy is dropped (searches
// rebuild the f16 copy on demand or stay on the exact paths).
int32_t grow(cs_index* h, uint64_t need_rows) {
    if (need_rows <= h->capacity) return CS_OK;
    // drain the device before the old buffers are copied and freed, or rows of an unfinished append would be lost
    if (h->ledger.stored()) CS_TRY(drain_appends(h));
    uint64_t cap = h->capacity ? h->capacity * 2 : 1024;
    if (cap < need_rows) cap = need_rows;
    GrowBuffers nb;
    const size_t words = (size_t)((cap + 31) / 32);
    hipError_t e = hipMalloc(&nb.nc, (size_t)cap * h->dim * sizeof(float));
    if (e != hipSuccess) return fail(CS_ERR_OOM, "hipMalloc(corpus, %llu rows) failed: %s", (unsigned long long)cap, hipGetErrorString(e));
    e = hipMalloc(&nb.nd, words * sizeof(uint32_t));
    if (e != hipSuccess) return fail(CS_ERR_OOM, "hipMalloc(dead bitmap) failed: %s", hipGetErrorString(e));
    e = hipMalloc(&nb.nn, (size_t)cap * sizeof(float));
    if (e != hipSuccess) return fail(CS_ERR_OOM, "hipMalloc(row norms) failed: %s", hipGetErrorString(e));
    bool drop_split = false, drop_q8 = false;
    size_t cap256 = 0;
    if (h->d_split) {
        // the f16 copy exists (the int8 copy does not serve): it grows with the corpus.  Without room for it, it is
        // dropped — searches then build it again on demand or stay on the exact paths; the int8 copy below does not
        // depend on it (whole 128-row tiles, an even number of them: 256-row blocks)
        cap256 = ((size_t)cap + 255) / 256 * 256;
        if (hipMalloc(&nb.ns, cap256 * h->dim * sizeof(_Float16)) != hipSuccess) {
            (void)hipGetLastError();
            nb.ns = nullptr;
            drop_split = true;
        } else if (h->split_rows) {
            CS_GROW_COPY(1, hipMemcpy(nb.ns, h->d_split, ((size_t)h->split_rows + 127) / 128 * 128 * h->dim * sizeof(_Float16),
                                      hipMemcpyDeviceToDevice));
        }
    }
    if (h->use_q8) {
        const size_t tiles = ((size_t)cap + 255) / 256 * 2;  // an even number: the 256-row tile kernel reads whole pairs
        const bool fault = cs_lab_env("CS_FAULT_INT8_ALLOC") != nullptr && h->capacity != 0;  // tests: the failure path
        if (fault || hipMalloc(&nb.n8, tiles * 128 * h->dim) != hipSuccess || hipMalloc(&nb.nm, tiles * sizeof(float4)) != hipSuccess) {
            (void)hipGetLastError();  // no room: no int8 copy from here on (the f16 copy, or the exact paths, serve)
            if (nb.n8) (void)hipFree(nb.n8);
            nb.n8 = nullptr; nb.nm = nullptr;
            drop_q8 = true;
        } else if (h->q8_rows) {
            CS_GROW_COPY(2, hipMemcpy(nb.n8, h->d_q8, (size_t)h->q8_rows * h->dim, hipMemcpyDeviceToDevice));
            CS_GROW_COPY(2, hipMemcpy(nb.nm, h->d_tmeta, (size_t)(h->q8_rows / 128) * sizeof(float4), hipMemcpyDeviceToDevice));
        }
    }
    CS_GROW_COPY(3, hipMemset(nb.nd, 0, words * sizeof(uint32_t)));
    if (h->normed_rows)
        CS_GROW_COPY(4, hipMemcpy(nb.nn, h->d_norms, (size_t)h->normed_rows * sizeof(float), hipMemcpyDeviceToDevice));
    if (h->ledger.stored()) {
        const std::vector<uint32_t>& dead = h->ledger.dead_words();
        CS_GROW_COPY(5, hipMemcpy(nb.nc, h->d_corpus, (size_t)h->ledger.stored() * h->dim * sizeof(float), hipMemcpyDeviceToDevice));
        CS_GROW_COPY(6, hipMemcpy(nb.nd, dead.data(), dead.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // ---- commit: nothing below can fail ----
    if (h->d_split) {
        (void)hipFree(h->d_split);
        h->d_split = nb.ns;
        nb.ns = nullptr;
        if (drop_split) { h->split_rows = 0; h->split_cap = 0; }
        else h->split_cap = cap256;
    }
    if (h->use_q8) {
        // the old, smaller buffers never survive a grow: a build that found them would convert tiles past their end
        if (h->d_q8) (void)hipFree(h->d_q8);
        if (h->d_tmeta) (void)hipFree(h->d_tmeta);
        h->d_q8 = nb.n8;
        h->d_tmeta = nb.nm;
        nb.n8 = nullptr; nb.nm = nullptr;
        if (drop_q8) { h->use_q8 = false; h->q8_rows = 0; }
    }
    if (h->d_norms) (void)hipFree(h->d_norms);
    h->d_norms = nb.nn;
    if (h->d_corpus) (void)hipFree(h->d_corpus);
    if (h->d_dead) (void)hipFree(h->d_dead);
    h->d_corpus = nb.nc;
    h->d_dead = nb.nd;
    nb.nn = nullptr; nb.nc = nullptr; nb.nd = nullptr;
    h->capacity = cap;
    return CS_OK;
}
#undef CS_GROW_COPY

// rows idx[0 .. n) of src (relative to it) -> dst rows 0 .. n, `dim` floats each
__global__ void __launch_bounds__(256)
gather_rows_kernel(const float* __restrict__ src, const uint32_t* __restrict__ idx, uint64_t n, uint32_t dim, float* __restrict__ dst) {
    const uint64_t total = n * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / dim;
        dst[i] = src[(size_t)idx[r] * dim + (i - r * dim)];
    }
}

// cs_index_build, when enough of the stored rows are tombstones: the live rows move to the front of the corpus in their order
// (chunk by chunk: a chunk's survivors are gathered straight into place when their destination lies wholly before the chunk,
// through a bounded staging buffer otherwise — never a second corpus), the row -> id table keeps their ids, and everything
// derived from the rows (norms, mean unit row, int8 / f16 filter copies) is rebuilt by the build that called this.  A search
// afterwards streams only live rows, and returns what it returned before: the same ids, the same cosines, bit for bit.
int32_t compact(cs_index* h) {
    const uint64_t live = h->ledger.live(), stored = h->ledger.stored();
    constexpr uint64_t CH = 1u << 18;  // rows per chunk (staging: 403 MB at dim 384)
    const uint64_t chunk = std::min<uint64_t>(CH, stored);
    struct Tmp {
        float* rows = nullptr; uint32_t* idx = nullptr;
        ~Tmp() { if (rows) (void)hipFree(rows); if (idx) (void)hipFree(idx); }
    } t;
    CS_HIP(hipMalloc(&t.rows, (size_t)chunk * h->dim * sizeof(float)));
    CS_HIP(hipMalloc(&t.idx, (size_t)chunk * sizeof(uint32_t)));
    std::vector<uint32_t> idx;
    idx.reserve((size_t)chunk);
    uint64_t dst = 0;
    for (uint64_t c0 = 0; c0 < stored; c0 += chunk) {
        const uint64_t c1 = std::min(stored, c0 + chunk);
        idx.clear();
        h->ledger.survivors(c0, c1, idx);
        const uint64_t cnt = idx.size();
        if (cnt == 0) continue;
        if (dst == c0 && cnt == c1 - c0) { dst += cnt; continue; }  // nothing deleted up to here: the rows are in place
        CS_HIP(hipMemcpyAsync(t.idx, idx.data(), (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, nullptr));
        const uint32_t blocks = (uint32_t)std::min<uint64_t>((cnt * h->dim + 255) / 256, (uint64_t)h->num_cus * 16);
        const bool direct = dst + cnt <= c0;  // the destination does not reach into the chunk being read
        hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, nullptr, h->d_corpus + (size_t)c0 * h->dim, t.idx, cnt, h->dim,
                           direct ? h->d_corpus + (size_t)dst * h->dim : t.rows);
        CS_HIP(hipGetLastError());
        if (!direct)
            CS_HIP(hipMemcpyAsync(h->d_corpus + (size_t)dst * h->dim, t.rows, (size_t)cnt * h->dim * sizeof(float), hipMemcpyDeviceToDevice, nullptr));
        CS_HIP(hipStreamSynchronize(nullptr));  // (idx is reused by the next chunk)
        dst += cnt;
    }
    if (dst != live) return fail(CS_ERR_HIP, "compaction moved %llu rows, expected %llu", (unsigned long long)dst, (unsigned long long)live);
    h->ledger.commit_reclaim();
    if (h->d_dead && h->capacity) CS_HIP(hipMemset(h->d_dead, 0, (size_t)((h->capacity + 31) / 32) * sizeof(uint32_t)));
    h->ids_uploaded = 0;
    // everything derived from the rows is rebuilt over the new storage order by the build that follows
    h->normed_rows = 0;
    h->q8_rows = 0;
    h->split_rows = 0;
    h->compactions += 1;
    return CS_OK;
}

int32_t check_append(cs_index* h, uint64_t n, uint32_t dim) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (dim != h->dim)  // store.rs:667-671
        return fail(CS_ERR_DIM_MISMATCH, "Embedding dimension mismatch: expected %u, got %u",
                    h->dim, dim);
    if (!h->ledger.can_append(n))
        return fail(CS_ERR_BAD_ARG, "id space exhausted: ids are u32 (store.rs:97)");
    return CS_OK;
}

void finish_append(cs_index* h, uint64_t n, uint32_t* out_ids) {
    const uint32_t start = h->ledger.append(n);
    if (out_ids)
        for (uint64_t i = 0; i < n; ++i) out_ids[i] = start + (uint32_t)i;  // store.rs:684
    if (n) h->built = false;  // store.rs:682
}

Workspace* acquire_pooled(cs_index* h) {
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->pool.empty()) {
        Workspace* w = h->pool.back();
        h->pool.pop_back();
        return w;
    }
    Workspace* w = new Workspace();
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return nullptr;
    }
    w->own_stream = true;
    return w;
}

void release_pooled(cs_index* h, Workspace* w) {
    std::lock_guard<std::mutex> lk(h->mu);
    h->pool.push_back(w);
}

Workspace* for_stream(cs_index* h, hipStream_t s) {
    std::lock_guard<std::mutex> lk(h->mu);
    const auto key = std::make_pair(s, std::this_thread::get_id());
    auto it = h->by_stream.find(key);
    if (it != h->by_stream.end()) return it->second;
    Workspace* w = new Workspace();
    w->stream = s;
    h->by_stream[key] = w;
    return w;
}

bool take_events(cs_index* h, Workspace* w, EventTriple* t) {
    if (!h->profile) return false;
    if (!w->free_events.empty()) {
        *t = w->free_events.back();
        w->free_events.pop_back();
        return true;
    }
    if (hipEventCreate(&t->e0) != hipSuccess) return false;
    if (hipEventCreate(&t->e1) != hipSuccess) return false;
    if (hipEventCreate(&t->e2) != hipSuccess) return false;
    return true;
}

// what every launch of one search shares; outputs are device pointers (any may be null)
struct SearchArgs {
    const ScanPlan& plan;
    const float* d_queries;
    uint32_t nq, k;
    uint64_t* d_keys; float* d_cos; uint32_t* d_ids; uint32_t* d_counts;
    hipStream_t stream;
    const uint32_t* d_dead;  // null when no row is tombstoned
};

int32_t close_timing(cs_index* h, const EventTriple& ev, hipStream_t stream) {
    CS_HIP(hipEventRecord(ev.e2, stream));
    std::lock_guard<std::mutex> lk(h->mu);
    h->pending.push_back(ev);
    return CS_OK;
}

// overflowed searches the device has reported since this workspace last looked: a strike against the int8 copy
// only when the search that overflowed read it (the exact-f32 batched path and the f16 filter share the word)
void fold_overflows(cs_index* h, Workspace* w) {
    if (!w->bs.h_mirror) return;
    const uint32_t seen = *reinterpret_cast<volatile uint32_t*>(w->bs.h_mirror);
    if (seen == w->mirror_seen) return;
    w->mirror_seen = seen;
    if (w->last_via_q8 && h->q8_active.load()) h->q8_strike();
}

// the exact list-based scan and its merge (gate: launch_scan)
int32_t list_scan(cs_index* h, Workspace* w, const SearchArgs& a, const uint32_t* gate) {
    CS_TRY(launch_scan(a.plan, h->d_corpus, h->ledger.stored(), h->dim, a.d_queries, a.nq, a.k, a.d_dead, h->row_ids(), w->d_partial,
                       a.stream, nullptr, false, gate));
    return launch_merge(w->d_partial, a.plan.blocks, a.nq, a.k, false, w->d_tmp_a, w->d_tmp_b, a.d_keys, a.d_cos, a.d_ids,
                        a.d_counts, a.stream, gate);
}

int32_t split_filter(cs_index* h, Workspace* w, const SearchArgs& a, const Q8View* q8) {
    return launch_scan_split(w->bs, w->qw, h->d_corpus, h->d_split, h->ledger.stored(), h->dim, a.d_queries, a.nq, a.k, a.d_dead,
                             h->row_ids(), a.d_keys, a.d_cos, a.d_ids, a.d_counts, a.stream, h->filter_margin, q8);
}

// After a batched search (filter or exact MFMA): a candidate buffer holds batched_cap(k) entries and a phase appends at
// most one per row, so it can only overflow over more rows than that (adversarial row order; thousands of near-duplicate
// rows).  Then the exact answer comes from a rerun.
int32_t settle_overflow(cs_index* h, Workspace* w, const SearchArgs& a, bool via_q8, bool may_sync, const EventTriple* ev) {
    const bool can_overflow = h->ledger.stored() > batched_cap(a.k);
    bool overflow = false, reran = false;
    if (!may_sync) {
        // Device API: never wait for the device.  Up to kGatedMaxQ queries, the exact list-based scan and
        // its merge are enqueued right behind the search with the overflow word as their gate: every
        // block exits at once unless the search overflowed (then they overwrite its outputs), so what
        // the caller's stream delivers is exact either way; cost when not taken ~3 near-empty launches.
        // Above that (hundreds of query passes would be enqueued) the sticky word is left for
        // cs_index_search_status().
        if (can_overflow && a.nq <= kGatedMaxQ) CS_TRY(list_scan(h, w, a, w->bs.d_overflow));
    } else if (can_overflow) {
        CS_TRY(w->read_overflow(a.stream, &overflow));
        if (overflow && via_q8) h->q8_strike();  // the int8 copy's band let too many rows through
        if (overflow && via_q8 && ensure_f16(h)) {
            // ... and the f16 copy (band 0.001; built now if this is the first time it is needed) answers this search
            // before the exact list-based scan is asked to
            w->last_via_q8 = false;
            CS_TRY(split_filter(h, w, a, nullptr));
            CS_TRY(w->read_overflow(a.stream, &overflow));
            // the rerun's first kernel has mirrored the count of overflowed searches, this one included: seen
            w->mirror_seen = *reinterpret_cast<volatile uint32_t*>(w->bs.h_mirror);
            reran = true;
        }
    }
    {
        std::lock_guard<std::mutex> lk(h->mu);
        h->batched_searches++;
        if (overflow) h->batched_fallbacks++;
        if (reran) h->q8_reruns++;
    }
    if (ev) CS_TRY(close_timing(h, *ev, a.stream));
    return overflow ? list_scan(h, w, a, nullptr) : CS_OK;  // overflowed: the exact list-based rerun
}

// Plans the search (search_route.hpp), resolves its filter copy and launches it on `stream`.
// h_queries_pinned != null: the queries are still in that pinned host buffer and d_queries is empty.
int32_t run_search(cs_index* h, Workspace* w, const ScanPlan& plan, const float* d_queries,
                   uint32_t nq, uint32_t k, uint64_t* d_keys, float* d_cos, uint32_t* d_ids,
                   uint32_t* d_counts, hipStream_t stream, const float* h_queries_pinned = nullptr,
                   bool may_sync = true) {
    EventTriple ev{};
    const bool timed = take_events(h, w, &ev);
    if (timed) CS_HIP(hipEventRecord(ev.e0, stream));
    const SearchShape shape{nq, k, h->dim, h->ledger.stored(), h->num_cus, h->ledger.stored() > 0 && h->normed_rows >= h->ledger.stored(), h->use_split,
                            batched_supported(h->dim), scan_prime_supported(h->dim), h_queries_pinned != nullptr,
                            (uint64_t)plan.blocks * plan.passes};
    // Which copy filters: the int8 one when it serves; else the f16 one, built here, once, if it is not there yet; with
    // neither (no room) the search takes the exact paths.  A strike can retire the int8 copy: the choice is made after it.
    bool via_q8 = false, have_copy = false;
    if (route_wants_filter(h->route, shape, q8_serves(h))) {
        fold_overflows(h, w);
        via_q8 = q8_serves(h);
        bool planes = false;
        CS_TRY(w->reserve_split_queries(nq, h->dim, via_q8, &planes));
        via_q8 = via_q8 && planes;  // no room for the int8 query planes: the f16 copy
        have_copy = via_q8 || ensure_f16(h);
    }
    const SearchRoute route = plan_route(h->route, shape, have_copy);
    w->qw.q_pinned = route.queries == QuerySource::PrepPinned ? h_queries_pinned : nullptr;
    if (route.queries == QuerySource::StreamPinned) d_queries = h_queries_pinned;
    if (route.queries == QuerySource::Copy)
        CS_HIP(hipMemcpyAsync(const_cast<float*>(d_queries), h_queries_pinned, (size_t)nq * h->dim * sizeof(float),
                              hipMemcpyHostToDevice, stream));
    const SearchArgs a{plan, d_queries, nq, k, d_keys, d_cos, d_ids, d_counts, stream, h->ledger.removed() ? h->d_dead : nullptr};
    if (route.path == SearchPath::Stream) {
        const ScanPrime* prime = nullptr;
        if (route.prime_rows) {
            const ScanPlan pp = plan_prime(route.prime_rows, h->dim, nq, k, h->num_cus);
            CS_TRY(w->reserve_prime(pp, nq));
            CS_TRY(launch_scan(pp, h->d_corpus, route.prime_rows, h->dim, d_queries, nq, k, a.d_dead, h->row_ids(), nullptr,
                               stream, &w->prime, true));
            prime = &w->prime;
        }
        CS_TRY(launch_scan(plan, h->d_corpus, h->ledger.stored(), h->dim, d_queries, nq, k, a.d_dead, h->row_ids(), w->d_partial,
                           stream, prime));
        if (timed) CS_HIP(hipEventRecord(ev.e1, stream));
        CS_TRY(launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, d_keys, d_cos, d_ids, d_counts,
                            stream));
        return timed ? close_timing(h, ev, stream) : CS_OK;
    }
    CS_TRY(w->reserve_batched(nq, k));
    w->last_via_q8 = via_q8;
    if (route.path == SearchPath::Filter) {
        Q8View q8;
        if (via_q8) {
            q8.d_q8 = h->d_q8; q8.d_tmeta = h->d_tmeta; q8.d_mu = h->d_mu; q8.rows = h->q8_rows;
            h->q8_searches.fetch_add(1);
        }
        CS_TRY(split_filter(h, w, a, &q8));
    } else {
        CS_TRY(launch_scan_batched(w->bs, h->d_corpus, h->d_norms, h->ledger.stored(), h->dim, d_queries, nq, k, a.d_dead, h->row_ids(),
                                   h->num_cus, d_keys, d_cos, d_ids, d_counts, stream));
    }
    if (timed) CS_HIP(hipEventRecord(ev.e1, stream));
    return settle_overflow(h, w, a, via_q8, may_sync, timed ? &ev : nullptr);
}

// The pinned queries of a host-buffer search -> w->d_queries, on the workspace's stream.
int32_t upload_queries(const cs_index* h, Workspace* w, uint32_t nq) {
    CS_HIP(hipMemcpyAsync(w->d_queries, w->h_queries, (size_t)nq * h->dim * sizeof(float), hipMemcpyHostToDevice, w->stream));
    return CS_OK;
}

// Upper bound of the live rows a mask allows (masked_plan.hpp allowed_bound): 0 = the search launches nothing.
uint64_t masked_bound(const cs_index* h, const uint32_t* allow, uint64_t allow_bits) {
    return allowed_bound(allow, allow_bits, h->ledger.id_base(), h->ledger.next_id(), h->ledger.live());
}

// Everything of a masked or scoped search behind its row list, on `stream`: the optional prime pass and the gathered scan
// over d_list[0, *d_len), then the shared merge -> the best k per query (outputs as launch_merge's, each optional).
// `rows` sized the plan: an upper bound of *d_len (a mask's popcount bound) or the length itself (a scope's).
int32_t run_row_list(cs_index* h, Workspace* w, const ScanPlan& plan, uint64_t rows, const uint32_t* d_list,
                     const uint32_t* d_len, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_keys, float* d_cos,
                     uint32_t* d_ids, uint32_t* d_counts, hipStream_t stream) {
    const uint64_t prime_rows = masked_prime_rows(h->route, rows, nq, k, h->dim, h->num_cus, scan_prime_supported(h->dim));
    const ScanPrime* prime = nullptr;
    if (prime_rows) {
        const ScanPlan pp = plan_prime(prime_rows, h->dim, nq, k, h->num_cus);
        CS_TRY(w->reserve_prime(pp, nq));
        CS_TRY(launch_scan_masked(pp, h->d_corpus, h->dim, d_list, d_len, d_queries, nq, k, h->row_ids(), nullptr, stream,
                                  &w->prime, true, prime_rows));
        prime = &w->prime;
    }
    CS_TRY(launch_scan_masked(plan, h->d_corpus, h->dim, d_list, d_len, d_queries, nq, k, h->row_ids(), w->d_partial,
                              stream, prime));
    return launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, d_keys, d_cos, d_ids, d_counts,
                        stream);
}

// A masked search (scan_masked.hip) on `stream`, for a mask whose bound (masked_bound) is > 0 and a plan sized by it: the
// row list, then run_row_list -> the best k keys per query in d_keys [nq][k].  `allow` is host memory that must stay
// valid until the stream has passed the search.
int32_t run_masked(cs_index* h, Workspace* w, const ScanPlan& plan, uint64_t bound, const float* d_queries, uint32_t nq,
                   uint32_t k, const uint32_t* allow, uint64_t allow_bits, uint64_t* d_keys, hipStream_t stream) {
    const MaskWindow win = mask_window(allow_bits, h->ledger.id_base(), h->ledger.next_id());
    const uint32_t nb = mask_list_blocks(h->ledger.stored());
    CS_TRY(w->reserve_masked(win.words, bound, nb));
    CS_HIP(hipMemcpyAsync(w->d_allow, allow + win.first_word, (size_t)win.words * sizeof(uint32_t), hipMemcpyHostToDevice,
                          stream));
    CS_TRY(launch_mask_rows(w->d_allow, win.lo, win.hi, h->ledger.removed() ? h->d_dead : nullptr, h->row_ids(), h->ledger.stored(),
                            w->d_mblocks, w->d_list, bound, stream));
    return run_row_list(h, w, plan, bound, w->d_list, w->d_mblocks + nb, d_queries, nq, k, d_keys, nullptr, nullptr, nullptr,
                        stream);
}

// ---- scopes (scope.hpp) ----------------------------------------------------------------------------

// Frees what the scope owns.  It reads nothing of the index or the shards (sc->index only tells the two kinds apart).
void scope_free(cs_scope* sc) {
    for (cs_scope* p : sc->parts) scope_free(p);
    if (sc->index) {
        DeviceGuard g(sc->device);
        if (sc->stream) { (void)hipStreamSynchronize(sc->stream); (void)hipStreamDestroy(sc->stream); }
        free_bufs(false, sc->d_ids, sc->d_list, sc->d_blocks, sc->d_blocked, sc->d_table);
        free_bufs(true, sc->h_len);
    }
    delete sc;
}

// Makes the scope's row list from its ids for the index as it stands (built), on the scope's stream (a remaking after
// the device has finished what was enqueued on it), waits for it and publishes length and generation.  The caller holds sc->mu and has the index's device current.
int32_t scope_make_list(cs_index* h, cs_scope* sc) {
    const uint64_t gen = h->build_gen.load();
    uint64_t live = 0;
    if (sc->n_ids) {
        const uint32_t nb = scope_list_blocks(sc->n_ids);
        // a remaking rewrites d_list and d_blocks: a device-form search of the earlier generation that is still only
        // enqueued on its caller's stream reads them, so the device's work is waited for first (once per build and scope)
        if (sc->generation) CS_HIP(hipDeviceSynchronize());
        CS_TRY(launch_scope_rows(sc->d_ids, sc->n_ids, h->ledger.removed() ? h->d_dead : nullptr, h->row_ids(), h->ledger.stored(),
                                 sc->d_blocks, sc->d_list, sc->n_ids, sc->stream));
        // a scope that can ever take the filter (it has a table): the blocked-rows bitmap over the store's rows as they
        // are now, and the host's view of the list, in the same read-back.  Without room for the bitmap the scope
        // simply keeps to the gathered scan.
        sc->filter_state = false;
        bool state = sc->d_table && h->ledger.stored() > 0;
        if (state) {
            const size_t words = (size_t)scope_blocked_words(h->ledger.stored());
            if (words > sc->blocked_words) {
                sc->blocked_words = 0;
                if (realloc_buf(sc->d_blocked, words) == hipSuccess) sc->blocked_words = words;
                else { (void)hipGetLastError(); state = false; }
            }
        }
        if (state) {
            CS_TRY(launch_scope_filter_state(sc->d_list, sc->d_blocks + nb, sc->n_ids, h->ledger.stored(), sc->d_blocked, sc->d_table,
                                             sc->stream));
            CS_HIP(hipMemcpyAsync(sc->h_len + 1, sc->d_table, sc->table_words * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                  sc->stream));
            CS_HIP(hipMemcpyAsync(sc->h_len + 1 + sc->table_words, sc->d_list,
                                  (size_t)scope_head_entries(sc->n_ids) * sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
        }
        CS_HIP(hipMemcpyAsync(sc->h_len, sc->d_blocks + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
        CS_HIP(hipStreamSynchronize(sc->stream));
        live = *sc->h_len;
        sc->filter_state = state && scope_filter_capable(h->dim, live);
        if (!sc->filter_state && sc->d_blocked) {  // everything fits phase 0 now: no bitmap is held for it
            free_bufs(false, sc->d_blocked);
            sc->blocked_words = 0;
        }
    }
    sc->live_rows = live;
    sc->generation = gen;
    sc->refreshes += 1;
    return CS_OK;
}

// ---- the making of a scope: cs_index_scope_create, _create_range and cs_scope_combine differ only in where the ids come from

cs_scope* new_index_scope(cs_index* h) {
    cs_scope* sc = new cs_scope();
    sc->index = h;
    sc->device = h->device;
    return sc;
}

// The buffers of a scope of n ids over h (and its stream, unless it has one); n == 0 holds nothing.  The index's device
// is current.
int32_t scope_alloc(cs_index* h, cs_scope* sc, uint64_t n) {
    sc->n_ids = n;
    if (!n) return CS_OK;
    if (!sc->stream) CS_HIP(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
    CS_HIP(realloc_buf(sc->d_ids, (size_t)n));
    CS_HIP(realloc_buf(sc->d_list, (size_t)n));
    CS_HIP(realloc_buf(sc->d_blocks, (size_t)scope_list_blocks(n) + 1));
    // a scope that can ever take the int8 filter keeps the stride table and reads more back per making
    const bool tables = h->use_q8 && scope_filter_capable(h->dim, n);
    if (tables) {
        sc->table_words = 1 + (size_t)scope_stride_entries(n);
        CS_HIP(realloc_buf(sc->d_table, sc->table_words));
    }
    CS_HIP(realloc_buf(sc->h_len, tables ? 1 + sc->table_words + (size_t)scope_head_entries(n) : 1, true));
    return CS_OK;
}

// The list of a scope whose ids are in place.  An index that is not built has rows the device does not know yet (the
// row -> id table is uploaded by the build): the list is then made by the first search, which needs that build.
int32_t scope_first_list(cs_index* h, cs_scope* sc) {
    std::lock_guard<std::mutex> lk(sc->mu);
    return h->built ? scope_make_list(h, sc) : CS_OK;
}

// cs_scope_combine over one index: the counting pass and the scan on the result's own stream, one read-back of the total
// that sizes the result exactly (scope_alloc, as a create call of that many ids), the ordered write, then the list as every
// scope gets it.  The inputs' d_ids and n_ids never change after their making, so nothing of a or b is locked.
int32_t scope_combine_one(const cs_scope* a, const cs_scope* b, int32_t op, cs_scope** out) {
    cs_index* h = a->index;
    DeviceGuard g(h->device);
    cs_scope* sc = new_index_scope(h);
    uint32_t* d_tiles = nullptr;
    const int32_t st = [&]() -> int32_t {
        const uint64_t na = a->n_ids, nb = b->n_ids;
        uint64_t n = 0;
        // short cut: an empty a, or an intersection with an empty b, is the empty scope; nothing is launched
        const bool empty = na == 0 ? (op != CS_SCOPE_OP_UNION || nb == 0) : (nb == 0 && op == CS_SCOPE_OP_INTERSECT);
        if (!empty) {
            CS_HIP(hipStreamCreateWithFlags(&sc->stream, hipStreamNonBlocking));
            const uint64_t nt = scope_ops_tiles(na, nb);
            CS_HIP(realloc_buf(d_tiles, (size_t)nt + 1));
            CS_TRY(launch_scope_ops_count(a->d_ids, na, b->d_ids, nb, op, d_tiles, sc->stream));
            uint32_t total = 0;
            CS_HIP(hipMemcpyAsync(&total, d_tiles + nt, sizeof(uint32_t), hipMemcpyDeviceToHost, sc->stream));
            CS_HIP(hipStreamSynchronize(sc->stream));
            // the counts are u32: only a union of every u32 id (2^32 of them) wraps, to 0, and a union of a non-empty
            // input is never empty
            if (op == CS_SCOPE_OP_UNION && total == 0)
                return fail(CS_ERR_BAD_ARG, "a scope holds at most 2^32 - 1 ids (ids are u32): the union names every id");
            n = total;
            if (!n) {  // an empty result holds what a create call of 0 ids holds: nothing, no stream either
                CS_HIP(hipStreamDestroy(sc->stream));
                sc->stream = nullptr;
            }
        }
        CS_TRY(scope_alloc(h, sc, n));
        if (n) {
            CS_TRY(launch_scope_ops_write(a->d_ids, na, b->d_ids, nb, op, d_tiles, sc->d_ids, n, sc->stream));
            CS_HIP(hipStreamSynchronize(sc->stream));
        }
        return scope_first_list(h, sc);
    }();
    free_bufs(false, d_tiles);
    if (st != CS_OK) {
        scope_free(sc);
        return st;
    }
    *out = sc;
    return CS_OK;
}

int32_t scope_part_read_ids(const cs_scope* sc, uint64_t first, uint64_t n, uint32_t* out_ids) {
    DeviceGuard g(sc->device);
    CS_HIP(hipMemcpy(out_ids, sc->d_ids + first, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return CS_OK;
}

}  // namespace

// The checks of a scoped search behind check_search's, then the refresh when one is due: *live = the list's length.
// fp != null (the host-buffer searches of nq queries, top-k): the search's route too — fp->ok says that it wants the
// int8 filter and holds its plan (scoped_filter_plan.hpp; host arithmetic over what the scope keeps, under its mutex).
// (fp, nq and k default to none: index_internal.hpp.)
int32_t cs::scope_ready(cs_index* h, cs_scope* sc, uint64_t* live, ScopedFilterPlan* fp, uint32_t nq, uint32_t k) {
    CS_TRY(check_scope_handle(h, sc));
    std::lock_guard<std::mutex> lk(sc->mu);
    if (scope_refresh_due(sc->generation, h->build_gen.load())) CS_TRY(scope_make_list(h, sc));
    *live = sc->live_rows;
    if (!fp) return CS_OK;
    *fp = ScopedFilterPlan();
    ScopedRouteIn in;
    in.mode = sc->route.load();
    in.q8_serves = q8_serves(h);
    if (in.mode == CS_SCOPE_ROUTE_GATHER || !in.q8_serves || !sc->filter_state) return CS_OK;
    const ScopedFilterPlan plan = plan_scoped_filter(h->dim, h->ledger.stored(), sc->list_view(), nq, k, h->q8_rows, true, cu_count(),
                                                     filter_knobs());
    in.plan_ok = plan.ok;
    in.live = sc->live_rows;
    in.span = plan.span;
    const SearchShape shape{nq, k, h->dim, sc->live_rows, h->num_cus, h->normed_rows >= h->ledger.stored(), h->use_split,
                            batched_supported(h->dim), scan_prime_supported(h->dim), true, 0};
    if (scoped_wants_filter(h->route, shape, in)) *fp = plan;
    return CS_OK;
}

namespace {

// The keys of a host-buffer scoped search, enqueued on the workspace's stream: the best k per query into d_keys [nq][k]
// (device-addressable).  The queries are in w->h_queries.  With a filter plan whose int8 query planes fit, the index's
// filter + exact refine runs over the plan's row ranges with the scope's bitmap where the tombstones go; an overflowed
// candidate buffer is settled here, on the host, by the exact rerun over the scope's list (the unscoped list scan would
// ignore the scope) — counted per scope, no strike against the int8 copy and no f16-copy stage.  Else the gathered scan.
int32_t run_scoped(cs_index* h, cs_scope* sc, Workspace* w, const ScanPlan& plan, uint64_t live, const ScopedFilterPlan& fp,
                   uint32_t nq, uint32_t k, uint64_t* d_keys) {
    const uint32_t* d_len = sc->d_blocks + scope_list_blocks(sc->n_ids);
    bool planes = false;
    if (fp.ok) CS_TRY(w->reserve_split_queries(nq, h->dim, true, &planes));
    if (!(fp.ok && planes)) {
        sc->gathered_searches.fetch_add(1);
        CS_TRY(upload_queries(h, w, nq));
        return run_row_list(h, w, plan, live, sc->d_list, d_len, w->d_queries, nq, k, d_keys, nullptr, nullptr, nullptr, w->stream);
    }
    sc->filter_searches.fetch_add(1);
    CS_TRY(w->reserve_batched(nq, k));
    w->qw.q_pinned = w->h_queries;  // the prep kernel reads the pinned queries and leaves the device copy
    w->last_via_q8 = false;         // (this search is no reading of the int8 copy in the strike bookkeeping)
    Q8View q8;
    q8.d_q8 = h->d_q8; q8.d_tmeta = h->d_tmeta; q8.d_mu = h->d_mu; q8.rows = h->q8_rows;
    CS_TRY(launch_scan_split(w->bs, w->qw, h->d_corpus, nullptr, h->ledger.stored(), h->dim, w->d_queries, nq, k, sc->d_blocked,
                             h->row_ids(), d_keys, nullptr, nullptr, nullptr, w->stream, h->filter_margin, &q8, &fp.plan,
                             sc->d_list));
    if (live <= batched_cap(k)) return CS_OK;  // a phase appends at most one candidate per allowed row
    bool overflow = false;
    CS_TRY(w->read_overflow(w->stream, &overflow));
    if (!overflow) return CS_OK;
    sc->overflow_reruns.fetch_add(1);
    // The overflow is the scope's alone.  Left in the workspace, word [0] would be folded into the device's count of
    // overflowed searches by the next filter search's first kernel and surface later as a strike against the int8 copy
    // (fold_overflows) and in the index's fallback total; word [1] is the sticky word of searches of more than
    // kGatedMaxQ queries, which no host-buffer search reads.  Both are cleared here, in stream order, behind the read.
    CS_HIP(hipMemsetAsync(w->bs.d_overflow, 0, 2 * sizeof(uint32_t), w->stream));
    return run_row_list(h, w, plan, live, sc->d_list, d_len, w->d_queries, nq, k, d_keys, nullptr, nullptr, nullptr, w->stream);
}

// ensure_groups for the class table: the index's side of a boosted search's BoostView (the call adds its weights).  No
// class assigned: a null table, every id CS_NO_CLASS.
int32_t ensure_classes(cs_index* h, BoostView* bv) {
    std::lock_guard<std::mutex> lk(h->classes_mu);
    *bv = BoostView{};
    bv->id_base = h->ledger.id_base();
    if (h->classes.assigned() == 0) return CS_OK;
    const uint64_t n = h->classes.size();
    if (n > h->classes_cap) {
        CS_HIP(hipDeviceSynchronize());  // a search that was only enqueued may still read the old table
        const uint64_t cap = std::max<uint64_t>(n, std::min<uint64_t>(2 * h->classes_cap, 0xffffffffull));
        h->classes_cap = 0;
        h->classes.uploaded(0);  // the new table holds nothing yet
        CS_HIP(realloc_buf(h->d_classes, (size_t)cap));
        h->classes_cap = cap;
    }
    uint64_t lo = 0, hi = 0;
    if (h->classes.pending(&lo, &hi))
        CS_HIP(hipMemcpy(h->d_classes + lo, h->classes.data() + lo, (size_t)(hi - lo) * sizeof(uint16_t), hipMemcpyHostToDevice));
    h->classes.uploaded(n);
    bv->classes = h->d_classes;
    bv->len = (uint32_t)n;
    return CS_OK;
}

// A grouped search (scan_grouped.hip) on `stream`: the capped scan over every stored row, then the capped merge -> the
// best k keys per query in d_keys [nq][k].
int32_t run_grouped(cs_index* h, Workspace* w, const GroupedPlan& plan, const GroupView& gv, const float* d_queries,
                    uint32_t nq, uint32_t k, uint64_t* d_keys, hipStream_t stream) {
    CS_TRY(launch_scan_grouped(plan, h->d_corpus, h->ledger.stored(), h->dim, d_queries, nq, k, h->ledger.removed() ? h->d_dead : nullptr,
                               h->row_ids(), gv, w->d_partial, stream));
    return launch_merge_grouped(plan, w->d_partial, nq, k, gv, w->d_tmp_a, w->d_tmp_b, d_keys, nullptr, nullptr, nullptr,
                                stream);
}

// run_grouped over a scope's row list d_list[0, *d_len) (live rows only; the plan was made for the list's length): the
// gathered capped scan, then the same capped merge.
int32_t run_grouped_list(cs_index* h, Workspace* w, const GroupedPlan& plan, const GroupView& gv, const uint32_t* d_list,
                         const uint32_t* d_len, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_keys,
                         hipStream_t stream) {
    CS_TRY(launch_scan_grouped_list(plan, h->d_corpus, h->dim, d_list, d_len, d_queries, nq, k, h->row_ids(), gv, w->d_partial,
                                    stream));
    return launch_merge_grouped(plan, w->d_partial, nq, k, gv, w->d_tmp_a, w->d_tmp_b, d_keys, nullptr, nullptr, nullptr,
                                stream);
}

// The prime pass of a boosted search over `rows` rows (every stored row, or a scope's list): by the streaming route's rule
// (masked_prime_rows), a boosted pass over the first rows that leaves w->prime.d_floor[q] below query q's k-th best b.
// -> w->prime, or null when the rule asks for none.
int32_t boosted_prime(cs_index* h, Workspace* w, uint64_t rows, const BoostView& bv, const uint32_t* d_list, const uint32_t* d_len,
                      const float* d_queries, uint32_t nq, uint32_t k, hipStream_t stream, const ScanPrime** prime) {
    *prime = nullptr;
    const uint64_t prime_rows = masked_prime_rows(h->route, rows, nq, k, h->dim, h->num_cus, scan_prime_supported(h->dim));
    if (!prime_rows) return CS_OK;
    const ScanPlan pp = plan_prime(prime_rows, h->dim, nq, k, h->num_cus);
    CS_TRY(w->reserve_prime(pp, nq));
    if (d_list)
        CS_TRY(launch_scan_boosted_list(pp, h->d_corpus, h->dim, d_list, d_len, d_queries, nq, k, h->row_ids(), bv, nullptr, stream,
                                        &w->prime, true, prime_rows));
    else
        CS_TRY(launch_scan_boosted(pp, h->d_corpus, prime_rows, h->dim, d_queries, nq, k, h->ledger.removed() ? h->d_dead : nullptr,
                                   h->row_ids(), bv, nullptr, stream, &w->prime, true));
    *prime = &w->prime;
    return CS_OK;
}

// A boosted search (scan_boosted.hip) on `stream`: the optional prime pass and the boosted scan over every stored row,
// then the ordinary merge -> the best k keys of (b, id) per query in d_keys [nq][k].
int32_t run_boosted(cs_index* h, Workspace* w, const ScanPlan& plan, const BoostView& bv, const float* d_queries, uint32_t nq,
                    uint32_t k, uint64_t* d_keys, hipStream_t stream) {
    const ScanPrime* prime = nullptr;
    CS_TRY(boosted_prime(h, w, h->ledger.stored(), bv, nullptr, nullptr, d_queries, nq, k, stream, &prime));
    CS_TRY(launch_scan_boosted(plan, h->d_corpus, h->ledger.stored(), h->dim, d_queries, nq, k, h->ledger.removed() ? h->d_dead : nullptr,
                               h->row_ids(), bv, w->d_partial, stream, prime));
    return launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, d_keys, nullptr, nullptr, nullptr, stream);
}

// run_boosted over a scope's row list d_list[0, *d_len) (live rows only; `rows` = the list's length, which sized the plan):
// the gathered boosted scan, then the same merge.
int32_t run_boosted_list(cs_index* h, Workspace* w, const ScanPlan& plan, uint64_t rows, const BoostView& bv, const uint32_t* d_list,
                         const uint32_t* d_len, const float* d_queries, uint32_t nq, uint32_t k, uint64_t* d_keys,
                         hipStream_t stream) {
    const ScanPrime* prime = nullptr;
    CS_TRY(boosted_prime(h, w, rows, bv, d_list, d_len, d_queries, nq, k, stream, &prime));
    CS_TRY(launch_scan_boosted_list(plan, h->d_corpus, h->dim, d_list, d_len, d_queries, nq, k, h->row_ids(), bv, w->d_partial,
                                    stream, prime));
    return launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, d_keys, nullptr, nullptr, nullptr, stream);
}

// The route's thresholds of a new index: RouteKnobs' defaults, or what the environment sets.
RouteKnobs route_knobs_from_env() {
    RouteKnobs r;
    if (const char* e = std::getenv("CS_FILTER_MIN_Q")) r.filter_min_q = std::max(1, std::atoi(e));
    if (const char* e = std::getenv("CS_FILTER_SINGLE_MIN_K")) {  // "0": one query never takes the filter (= CS_ROUTE_STREAM)
        r.single_filter_min_k = (uint32_t)std::atol(e);
        if (r.single_filter_min_k == 0) r.single_route = CS_ROUTE_STREAM;
    }
    if (const char* e = std::getenv("CS_FILTER_SINGLE_MIN_ROWS")) r.single_int8_min_rows = (uint64_t)std::atoll(e);
    if (const char* e = std::getenv("CS_FILTER_SINGLE_MIN_ROWS_LONG")) r.single_int8_min_rows_long = (uint64_t)std::atoll(e);
    if (const char* e = cs_lab_env("CS_FILTER_FEW_MIN_ROWS")) r.few_queries_min_rows = r.few_queries_min_rows_short = (uint64_t)std::atoll(e);
    if (const char* e = std::getenv("CS_SINGLE_BATCHED_MAX_ROWS")) r.single_batched_max_rows = (uint64_t)std::atoll(e);
    if (const char* e = std::getenv("CS_SCAN_PRIME_MIN_K")) r.prime_min_k = (uint32_t)std::atol(e);  // 0 = off
    if (const char* e = std::getenv("CS_SCAN_PRIME_MIN_ROWS")) r.prime_min_rows = (uint64_t)std::atoll(e);
    if (const char* e = std::getenv("CS_SCAN_PRIME_ROWS")) r.prime_rows = (uint64_t)std::atoll(e);
    if (const char* e = std::getenv("CS_SCOPE_FILTER_MAX_SPAN")) r.scope_span_single = r.scope_span_few = r.scope_span_many = std::atof(e);
    return r;
}

// ---- the host-buffer searches' frame ------------------------------------------------------------------
// Where a host-buffer search leaves its answer: nq lists [nq][k] with counts[nq], or (variants) the nq lists merged into
// one list [k] with counts[0] = its length and the optional high-confidence flag (cs_index_search_variants).
// `capped` (a grouped variants search): the group table the variants are merged under — every per-variant list is a capped
// list and the merge caps again (launch_merge_variants_grouped); null: the plain variants merge.
// `boosted` (a boosted search): the keys carry b, which goes to `cos`; the winners' cosines, which the kind's enqueue step
// leaves in the pinned w->h_winner_cos, go to `winner_cos`; each of the four outputs may then be null.
// `boosted` with `variants` (a boosted search over query variants): score, cos, count and flag together.  The kind's
// enqueue step merges the variants itself (keys of b, so the merge's own cosine predicate would read b) and leaves the ONE
// list's keys in the pinned `keys` it is handed and the winners' cosines in w->h_winner_cos; count and flag are taken
// from those after the synchronisation (confident_list), and high_confidence may be null like the rest.
struct HostAnswer {
    float* cos; uint32_t* ids; uint32_t* counts; int32_t* high_confidence;
    bool variants;
    const GroupView* capped = nullptr;
    bool boosted = false;
    float* winner_cos = nullptr;
};

// unpack_keys (common.hpp) for a boosted answer: every output optional, and the second float of a slot from `cos`.
void unpack_boosted(const uint64_t* keys, const float* cos, uint32_t nq, uint32_t k, const HostAnswer& out) {
    for (uint32_t q = 0; q < nq; ++q) {
        uint32_t c = 0;
        for (size_t j = (size_t)q * k; j < (size_t)(q + 1) * k; ++j) {
            c += keys[j] != 0;
            if (out.cos) out.cos[j] = keys[j] ? key_cos(keys[j]) : 0.0f;
            if (out.winner_cos) out.winner_cos[j] = keys[j] ? cos[j] : 0.0f;
            if (out.ids) out.ids[j] = keys[j] ? key_id(keys[j]) : 0xFFFFFFFFu;
        }
        if (out.counts) out.counts[q] = c;
    }
}

// The high-confidence predicate of cs_index_search_variants (mod.rs:601-611) on a list of `count` cosines, best first: the
// list is not empty and the distance (1 - cos) / 2 of each of its first five entries is below 0.15, in f32.
bool confident_list(const float* cos, uint32_t count) {
    const uint32_t want = std::min<uint32_t>(count, 5);
    for (uint32_t j = 0; j < want; ++j)
        if (!((1.0f - cos[j]) * 0.5f < 0.15f)) return false;
    return count > 0;
}

// The argument checks every host-buffer search starts with, in this order.
int32_t check_host_search(const cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, const HostAnswer& out) {
    CS_TRY(check_search(h, nq, dim, k));
    if (out.variants && nq > CS_MAX_VARIANTS)
        return fail(CS_ERR_BAD_ARG, "at most %u query variants per call, got %u", CS_MAX_VARIANTS, nq);
    if (!queries || !out.cos || !out.ids || !out.counts) return fail(CS_ERR_BAD_ARG, "null buffer");
    return CS_OK;
}

// The empty answer (nothing the kind may return is stored: no launch, no workspace): every slot as unpack_keys leaves an
// empty one.
int32_t empty_answer(uint32_t nq, uint32_t k, const HostAnswer& out) {
    const size_t lists = out.variants ? 1 : nq;
    for (size_t i = 0; i < lists * k; ++i) {
        if (out.cos) out.cos[i] = 0.0f;
        if (out.winner_cos) out.winner_cos[i] = 0.0f;
        if (out.ids) out.ids[i] = 0xFFFFFFFFu;
    }
    if (out.counts) memset(out.counts, 0, lists * sizeof(uint32_t));
    if (out.variants && out.high_confidence) *out.high_confidence = 0;
    return CS_OK;
}

// One host-buffer search on a pooled workspace (own stream), for arguments that passed the checks: room for the kind's
// plan, the queries into w->h_queries, then enqueue(w, keys) puts the kind's launches on w->stream — the best k keys per
// query go to `keys`, and whether the queries are copied to the device is the kind's business.  queries == null: the kind's
// enqueue step produces the queries on the device (w->d_queries) itself, and w->h_queries is left alone.  Lists: keys = the pinned
// w->h_keys, the last kernel writes the packed keys straight into it (device-addressable, coherent): no D2H copy call.
// Variants: the per-variant lists stay in HBM (w->d_keys) and the merge kernel — the kind's: the plain variants merge, or
// the capped one when the answer carries a group table — writes the <= k survivors and the two scalars into pinned memory.  One stream sync either way, then the host unpacks.  A template, not std::function: nothing
// on this path allocates.
template <class Enqueue>
int32_t host_search(cs_index* h, const float* queries, uint32_t nq, uint32_t k, size_t partial_keys, size_t merge_keys,
                    const HostAnswer& out, Enqueue&& enqueue) {
    Workspace* w = acquire_pooled(h);
    if (!w) return fail(CS_ERR_HIP, "could not create a HIP stream");
    const int32_t s = [&]() -> int32_t {
        CS_TRY(w->reserve(partial_keys, merge_keys, nq, h->dim, k, true));
        const bool merge_here = out.variants && !out.boosted;  // a boosted kind merges its variants itself
        if (merge_here && !w->h_variant_meta) CS_HIP(hipHostMalloc(&w->h_variant_meta, 2 * sizeof(uint32_t)));
        if (queries) memcpy(w->h_queries, queries, (size_t)nq * h->dim * sizeof(float));
        CS_TRY(enqueue(w, merge_here ? w->d_keys : w->h_keys));
        if (merge_here && out.capped)
            CS_TRY(launch_merge_variants_grouped(w->d_keys, nq, k, *out.capped, w->d_tmp_a, w->d_tmp_b, w->h_keys, nullptr,
                                                 nullptr, w->h_variant_meta, w->h_variant_meta + 1, w->stream));
        else if (merge_here)
            CS_TRY(launch_merge_variants(w->d_keys, nq, k, k, w->h_keys, nullptr, nullptr, w->h_variant_meta,
                                         w->h_variant_meta + 1, w->stream));
        CS_HIP(hipStreamSynchronize(w->stream));
        if (out.boosted) unpack_boosted(w->h_keys, w->h_winner_cos, out.variants ? 1 : nq, k, out);
        else unpack_keys(w->h_keys, out.variants ? 1 : nq, k, out.cos, out.ids, out.variants ? nullptr : out.counts);
        if (merge_here) {
            *out.counts = w->h_variant_meta[0];
            if (out.high_confidence) *out.high_confidence = (int32_t)w->h_variant_meta[1];
        } else if (out.variants && out.high_confidence) {  // boosted: the list is best first, its empty slots last
            uint32_t count = 0;
            while (count < k && w->h_keys[count]) ++count;
            *out.high_confidence = confident_list(w->h_winner_cos, count) ? 1 : 0;
        }
        return CS_OK;
    }();
    release_pooled(h, w);
    return s;
}

// The plain search.  Variants: exact without a host round trip (<= 16 queries carry the gated rerun).
int32_t search_all(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, const HostAnswer& out) {
    CS_TRY(check_host_search(h, queries, nq, dim, k, out));
    DeviceGuard g(h->device);
    const ScanPlan plan = plan_scan(h->ledger.stored(), h->dim, nq, k, h->num_cus);
    return host_search(h, queries, nq, k, plan.partial_keys, plan.merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        return run_search(h, w, plan, w->d_queries, nq, k, keys, nullptr, nullptr, nullptr, w->stream, w->h_queries,
                          /*may_sync=*/!out.variants);
    });
}

int32_t search_masked(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, const uint32_t* allow,
                      uint64_t allow_bits, const HostAnswer& out) {
    CS_TRY(check_host_search(h, queries, nq, dim, k, out));
    if (!allow && allow_bits) return fail(CS_ERR_BAD_ARG, "allow is null");
    const uint64_t bound = masked_bound(h, allow, allow_bits);
    if (bound == 0) return empty_answer(nq, k, out);  // nothing allowed is stored
    DeviceGuard g(h->device);
    const ScanPlan plan = plan_scan(bound, h->dim, nq, k, h->num_cus);  // the grid follows the allowed rows
    return host_search(h, queries, nq, k, plan.partial_keys, plan.merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        CS_TRY(upload_queries(h, w, nq));
        return run_masked(h, w, plan, bound, w->d_queries, nq, k, allow, allow_bits, keys, w->stream);
    });
}

int32_t search_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                      const HostAnswer& out) {
    CS_TRY(check_host_search(h, queries, nq, dim, k, out));
    DeviceGuard g(h->device);
    uint64_t live = 0;
    ScopedFilterPlan fp;
    CS_TRY(scope_ready(h, scope, &live, &fp, nq, k));
    if (live == 0) return empty_answer(nq, k, out);  // nothing of the scope is stored
    const ScanPlan plan = plan_scan(live, h->dim, nq, k, h->num_cus);  // the grid follows the list's exact length
    // (an overflow of the filter route is settled inside run_scoped, before a variants' merge)
    return host_search(h, queries, nq, k, plan.partial_keys, plan.merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        return run_scoped(h, scope, w, plan, live, fp, nq, k, keys);
    });
}

// The grouped searches: over the whole store (scope_given false: the capped scan over every stored row) or over a scope's
// row list (the gathered capped scan, always: the int8 filter's threshold is the uncapped k-th, so no filter plan is asked
// for), one list per query or the variants merged under the cap.
int32_t search_grouped(cs_index* h, bool scope_given, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                       uint32_t per_group, HostAnswer out) {
    CS_TRY(check_host_search(h, queries, nq, dim, k, out));
    if (per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    DeviceGuard g(h->device);
    uint64_t rows = h->ledger.stored();
    if (scope_given) {
        CS_TRY(scope_ready(h, scope, &rows));
        if (rows == 0) return empty_answer(nq, k, out);  // nothing of the scope is stored
    }
    GroupView gv;
    CS_TRY(ensure_groups(h, per_group, &gv));
    if (out.variants) out.capped = &gv;
    const GroupedPlan plan = plan_grouped(rows, h->dim, nq, k, h->num_cus);  // a scope: the grid follows the list's length
    const size_t merge_keys = std::max(plan.merge_keys, out.variants ? grouped_variants_tmp_keys(nq, k) : (size_t)0);
    return host_search(h, queries, nq, k, plan.partial_keys, merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        CS_TRY(upload_queries(h, w, nq));
        if (!scope_given) return run_grouped(h, w, plan, gv, w->d_queries, nq, k, keys, w->stream);
        scope->gathered_searches.fetch_add(1);
        return run_grouped_list(h, w, plan, gv, scope->d_list, scope->d_blocks + scope_list_blocks(scope->n_ids), w->d_queries, nq,
                                k, keys, w->stream);
    });
}

// The call's weight table checked: n_classes entries, each finite and in [0, 65536] (so b stays finite and no key of a
// live row is a NaN's).  *wmin / *wmax: the table's extremes widened to hold 1, the weight of a row without a class.
int32_t check_weights(const float* weights, uint32_t n_classes, float* wmin, float* wmax) {
    *wmin = *wmax = 1.0f;
    if (n_classes > CS_MAX_CLASSES) return fail(CS_ERR_BAD_ARG, "n_classes must be at most %u, got %u", CS_MAX_CLASSES, n_classes);
    for (uint32_t i = 0; weights && i < n_classes; ++i) {
        const float x = weights[i];
        if (!(x >= 0.0f && x <= 65536.0f))  // NaN fails both
            return fail(CS_ERR_BAD_ARG, "weights[%u] = %g: a weight must be finite and in [0, 65536]", i, (double)x);
        *wmin = std::min(*wmin, x);
        *wmax = std::max(*wmax, x);
    }
    return CS_OK;
}

// The boosted searches (scan_boosted.hip): over the whole store (scope_given false: the boosted scan over every stored
// row) or over a scope's row list (the gathered boosted scan, always: the int8 filter's threshold is a cosine's, not a
// weighted score's).  The call's weights travel in its workspace, never in the index: concurrent calls with different
// tables do not meet.  Behind the merge the cosine pass recovers the winners' cosines and hands keys and cosines to pinned
// memory: one stream sync, no further round trip.
int32_t search_boosted(cs_index* h, bool scope_given, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                       const float* weights, uint32_t n_classes, float* out_score, float* out_cos, uint32_t* out_ids,
                       uint32_t* out_counts) {
    CS_TRY(check_search(h, nq, dim, k));
    if (!queries) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (!out_score && !out_cos && !out_ids && !out_counts) return fail(CS_ERR_BAD_ARG, "no output buffer given");
    if (!weights) n_classes = 0;
    float wmin = 1.0f, wmax = 1.0f;
    CS_TRY(check_weights(weights, n_classes, &wmin, &wmax));
    HostAnswer out{out_score, out_ids, out_counts, nullptr, false};
    out.boosted = true;
    out.winner_cos = out_cos;
    DeviceGuard g(h->device);
    uint64_t rows = h->ledger.stored();
    if (scope_given) CS_TRY(scope_ready(h, scope, &rows));
    if (rows == 0) return empty_answer(nq, k, out);  // nothing the call may return is stored
    BoostView bv;
    CS_TRY(ensure_classes(h, &bv));
    bv.wmin = wmin;
    bv.wmax = wmax;
    const ScanPlan plan = plan_scan(rows, h->dim, nq, k, h->num_cus);  // a scope: the grid follows the list's length
    return host_search(h, queries, nq, k, plan.partial_keys, plan.merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        CS_TRY(w->reserve_boosted(nq, k, n_classes));
        CS_TRY(upload_queries(h, w, nq));
        if (n_classes) {
            memcpy(w->h_weights, weights, n_classes * sizeof(float));
            CS_HIP(hipMemcpyAsync(w->d_weights, w->h_weights, n_classes * sizeof(float), hipMemcpyHostToDevice, w->stream));
            bv.weights = w->d_weights;
            bv.n_classes = n_classes;
        }
        if (!scope_given) CS_TRY(run_boosted(h, w, plan, bv, w->d_queries, nq, k, w->d_keys, w->stream));
        else {
            scope->gathered_searches.fetch_add(1);
            CS_TRY(run_boosted_list(h, w, plan, rows, bv, scope->d_list, scope->d_blocks + scope_list_blocks(scope->n_ids), w->d_queries,
                                    nq, k, w->d_keys, w->stream));
        }
        return launch_boosted_cos(h->d_corpus, h->ledger.stored(), h->dim, w->d_queries, nq, k, h->row_ids(), w->d_keys, keys,
                                  w->h_winner_cos, w->stream);
    });
}

// The boosted searches over query variants (cs_index_search_variants_boosted and its scoped / grouped forms): one list of
// the rows' best b over the nq variants, uncapped (per_group null) or under the per-file cap.  Per variant a list of b —
// run_boosted / run_boosted_list with their prime pass, or under the cap the boosted capped scan and the capped merge
// (scan_boosted_grouped.hip) — then the de-duplicating variants merge over those keys, which caps at every level (under a
// GroupView that caps nothing it is a plain de-duplicating merge), then the winners' cosines over all variants.  The
// scoped forms take the gathered scans, always.  Count and flag: host_search, from the keys and the cosines.
int32_t search_variants_boosted(cs_index* h, bool scope_given, cs_scope* scope, const uint32_t* per_group, const float* queries,
                                uint32_t nq, uint32_t dim, uint32_t k, const float* weights, uint32_t n_classes, float* out_score,
                                float* out_cos, uint32_t* out_ids, uint32_t* out_count, int32_t* out_high_confidence) {
    CS_TRY(check_search(h, nq, dim, k));
    if (nq > CS_MAX_VARIANTS) return fail(CS_ERR_BAD_ARG, "at most %u query variants per call, got %u", CS_MAX_VARIANTS, nq);
    if (!queries) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (!out_score && !out_cos && !out_ids && !out_count && !out_high_confidence)
        return fail(CS_ERR_BAD_ARG, "no output buffer given");
    if (per_group && *per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    if (!weights) n_classes = 0;
    float wmin = 1.0f, wmax = 1.0f;
    CS_TRY(check_weights(weights, n_classes, &wmin, &wmax));
    HostAnswer out{out_score, out_ids, out_count, out_high_confidence, true};
    out.boosted = true;
    out.winner_cos = out_cos;
    DeviceGuard g(h->device);
    uint64_t rows = h->ledger.stored();
    if (scope_given) CS_TRY(scope_ready(h, scope, &rows));
    if (rows == 0) return empty_answer(nq, k, out);  // nothing the call may return is stored
    BoostView bv;
    CS_TRY(ensure_classes(h, &bv));
    bv.wmin = wmin;
    bv.wmax = wmax;
    GroupView gv;  // as it stands it caps nothing
    if (per_group) CS_TRY(ensure_groups(h, *per_group, &gv));
    // a scope: the grids follow the list's length
    const ScanPlan plan = plan_scan(rows, h->dim, nq, k, h->num_cus);
    const GroupedPlan gplan = plan_grouped(rows, h->dim, nq, k, h->num_cus);
    const size_t partial_keys = per_group ? gplan.partial_keys : plan.partial_keys;
    const size_t merge_keys = std::max(per_group ? gplan.merge_keys : plan.merge_keys, grouped_variants_tmp_keys(nq, k));
    return host_search(h, queries, nq, k, partial_keys, merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        CS_TRY(w->reserve_boosted_variants(k, n_classes));
        CS_TRY(upload_queries(h, w, nq));
        if (n_classes) {
            memcpy(w->h_weights, weights, n_classes * sizeof(float));
            CS_HIP(hipMemcpyAsync(w->d_weights, w->h_weights, n_classes * sizeof(float), hipMemcpyHostToDevice, w->stream));
            bv.weights = w->d_weights;
            bv.n_classes = n_classes;
        }
        const uint32_t* d_list = scope_given ? scope->d_list : nullptr;
        const uint32_t* d_len = scope_given ? scope->d_blocks + scope_list_blocks(scope->n_ids) : nullptr;
        if (scope_given) scope->gathered_searches.fetch_add(1);
        if (per_group) {
            CS_TRY(launch_scan_boosted_grouped(gplan, h->d_corpus, h->ledger.stored(), h->dim, d_list, d_len, w->d_queries, nq, k,
                                               h->ledger.removed() ? h->d_dead : nullptr, h->row_ids(), bv, gv, w->d_partial,
                                               w->stream));
            CS_TRY(launch_merge_grouped(gplan, w->d_partial, nq, k, gv, w->d_tmp_a, w->d_tmp_b, w->d_keys, nullptr, nullptr, nullptr,
                                        w->stream));
        } else if (!scope_given) CS_TRY(run_boosted(h, w, plan, bv, w->d_queries, nq, k, w->d_keys, w->stream));
        else CS_TRY(run_boosted_list(h, w, plan, rows, bv, d_list, d_len, w->d_queries, nq, k, w->d_keys, w->stream));
        // the merge's decode of "cos" would yield b and its flag would read b: neither is asked for here
        CS_TRY(launch_merge_variants_grouped(w->d_keys, nq, k, gv, w->d_tmp_a, w->d_tmp_b, w->d_merged, nullptr, nullptr, nullptr,
                                             nullptr, w->stream));
        return launch_boosted_variants_cos(h->d_corpus, h->ledger.stored(), h->dim, w->d_queries, nq, k, h->row_ids(), w->d_merged,
                                           keys, w->h_winner_cos, w->stream);
    });
}

// The similar scan and its merge over every stored row: the SCAN route, and the exact answer of a FILTER-route call whose
// candidate buffer overflowed (never list_scan, which knows no exclusions).
int32_t similar_scan(cs_index* h, Workspace* w, const ScanPlan& plan, uint32_t nq, uint32_t k, const GroupView& gv,
                     const SimilarView& sv, uint64_t* keys) {
    CS_TRY(launch_scan_similar(plan, h->d_corpus, h->ledger.stored(), h->dim, w->d_queries, nq, k,
                               h->ledger.removed() ? h->d_dead : nullptr, h->row_ids(), gv, sv, w->d_partial, w->stream));
    return launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, keys, nullptr, nullptr, nullptr, w->stream);
}

// An unscoped similar-chunk search whose source rows are gathered in w->d_queries: plans its route (similar_route.hpp) and
// enqueues it.  FILTER: the ordinary search's filter on the copy run_search would choose — the int8 copy when it serves and
// its query planes fit, else the f16 copy (ensure_f16) — with the similar refine and fold (scan_similar_filter.hip); when a
// copy or the filter's buffers cannot be had ("no room") the call scans and counts as a scan.  The overflow word is read
// here, on the host; an overflowed candidate buffer — usually the excluded file's doing, not the copy's: its rows all beat
// the k-th best of the others — is settled by the similar scan into the same outputs, with no f16 rerun.
// A similar search never strikes the int8 copy and never moves the ordinary searches' counters: it does not call q8_strike,
// it is no reading of the int8 copy in the workspace's bookkeeping (last_via_q8), and its overflow word is cleared in stream
// order behind the read (as run_scoped clears a scope's), so the next search's prep kernel on this pooled workspace folds
// nothing into the device's count of overflowed searches and mirrors nothing new: fold_overflows has nothing to charge to
// whichever ordinary search runs here later.  What EARLIER ordinary searches left in the mirror is folded first, against them.
int32_t run_similar(cs_index* h, Workspace* w, const ScanPlan& plan, uint32_t nq, uint32_t k, const GroupView& gv,
                    const SimilarView& sv, uint64_t* keys) {
    const int32_t forced = h->similar_route.load();
    const uint64_t stored = h->ledger.stored();
    const SearchShape shape{nq, k, h->dim, stored, h->num_cus, stored > 0 && h->normed_rows >= stored, h->use_split,
                            batched_supported(h->dim), scan_prime_supported(h->dim), false, (uint64_t)plan.blocks * plan.passes};
    const bool serves = q8_serves(h);
    bool via_q8 = false, have_copy = false;
    if (similar_wants_filter(h->route, shape, serves, false, forced)) {
        fold_overflows(h, w);
        via_q8 = q8_serves(h);
        bool planes = false;
        int32_t room = w->reserve_split_queries(nq, h->dim, via_q8, &planes);
        via_q8 = via_q8 && planes;  // no room for the int8 query planes: the f16 copy
        if (room == CS_OK && (via_q8 || ensure_f16(h))) {
            room = w->reserve_batched(nq, k);
            have_copy = room == CS_OK;
        }
        if (room != CS_OK && room != CS_ERR_OOM) return room;
        if (room == CS_ERR_OOM) (void)hipGetLastError();  // no room: the scan answers
    }
    if (plan_similar_route(h->route, shape, serves, have_copy, false, forced) != SimilarRoute::Filter) {
        h->similar_scan_searches.fetch_add(1);
        return similar_scan(h, w, plan, nq, k, gv, sv, keys);
    }
    w->qw.q_pinned = nullptr;  // the gathered rows are device memory (QuerySource::Device)
    w->last_via_q8 = false;
    Q8View q8;
    if (via_q8) { q8.d_q8 = h->d_q8; q8.d_tmeta = h->d_tmeta; q8.d_mu = h->d_mu; q8.rows = h->q8_rows; }
    const SimilarRefine refine{sv, gv};
    CS_TRY(launch_scan_split(w->bs, w->qw, h->d_corpus, h->d_split, stored, h->dim, w->d_queries, nq, k,
                             h->ledger.removed() ? h->d_dead : nullptr, h->row_ids(), keys, nullptr, nullptr, nullptr, w->stream,
                             h->filter_margin, &q8, nullptr, nullptr, &refine));
    h->similar_filter_searches.fetch_add(1);
    if (stored <= batched_cap(k)) return CS_OK;  // a phase appends at most one candidate per row
    bool overflow = false;
    CS_TRY(w->read_overflow(w->stream, &overflow));
    if (!overflow) return CS_OK;
    h->similar_filter_fallbacks.fetch_add(1);
    CS_HIP(hipMemsetAsync(w->bs.d_overflow, 0, 2 * sizeof(uint32_t), w->stream));
    return similar_scan(h, w, plan, nq, k, gv, sv, keys);
}

// The scope's gathered similar scan and its merge: the GATHER route of a scoped similar-chunk search, and the exact answer
// of a FILTER-route call whose candidate buffer overflowed (never run_row_list, which knows no exclusions).
int32_t similar_list_scan(cs_index* h, cs_scope* sc, Workspace* w, const ScanPlan& plan, uint32_t nq, uint32_t k,
                          const GroupView& gv, const SimilarView& sv, uint64_t* keys) {
    CS_TRY(launch_scan_similar_list(plan, h->d_corpus, h->dim, sc->d_list, sc->d_blocks + scope_list_blocks(sc->n_ids), w->d_queries,
                                    nq, k, h->row_ids(), gv, sv, w->d_partial, w->stream));
    return launch_merge(w->d_partial, plan.blocks, nq, k, false, w->d_tmp_a, w->d_tmp_b, keys, nullptr, nullptr, nullptr, w->stream);
}

// A scoped similar-chunk search whose source rows are gathered in w->d_queries: run_scoped's sequence with run_similar's
// query handling.  With a filter plan (scope_ready: the scope's route, scoped_wants_filter as for the ordinary scoped search)
// whose int8 query planes and buffers fit, the index's filter runs over the plan's row ranges with the scope's bitmap where
// the tombstones go and the similar refine and fold (scan_similar_filter.hip; phase 0 in its list form); "no room" anywhere
// quietly takes the gathered scan and counts as gathered.  An overflowed candidate buffer — the excluded file's doing, as in
// run_similar — is settled here by the gathered similar scan into the same keys, counted per scope.  No strike against the
// int8 copy, no f16 stage, none of the index's counters: last_via_q8 is false and words [0] and [1] of the overflow state are
// cleared in stream order behind the read, as run_scoped clears them.
int32_t run_similar_scoped(cs_index* h, cs_scope* sc, Workspace* w, const ScanPlan& plan, uint64_t live, const ScopedFilterPlan& fp,
                           uint32_t nq, uint32_t k, const GroupView& gv, const SimilarView& sv, uint64_t* keys) {
    bool room = false;
    if (fp.ok) {
        bool planes = false;
        int32_t rc = w->reserve_split_queries(nq, h->dim, true, &planes);
        if (rc == CS_OK && planes) rc = w->reserve_batched(nq, k);
        if (rc != CS_OK && rc != CS_ERR_OOM) return rc;
        if (rc == CS_ERR_OOM) (void)hipGetLastError();  // no room: the gathered scan answers
        room = rc == CS_OK && planes;
    }
    if (!room) {
        sc->gathered_searches.fetch_add(1);
        return similar_list_scan(h, sc, w, plan, nq, k, gv, sv, keys);
    }
    sc->filter_searches.fetch_add(1);
    w->qw.q_pinned = nullptr;  // the gathered rows are device memory (QuerySource::Device)
    w->last_via_q8 = false;    // (this search is no reading of the int8 copy in the strike bookkeeping)
    Q8View q8;
    q8.d_q8 = h->d_q8; q8.d_tmeta = h->d_tmeta; q8.d_mu = h->d_mu; q8.rows = h->q8_rows;
    const SimilarRefine refine{sv, gv};
    CS_TRY(launch_scan_split(w->bs, w->qw, h->d_corpus, nullptr, h->ledger.stored(), h->dim, w->d_queries, nq, k, sc->d_blocked,
                             h->row_ids(), keys, nullptr, nullptr, nullptr, w->stream, h->filter_margin, &q8, &fp.plan, sc->d_list,
                             &refine));
    if (live <= batched_cap(k)) return CS_OK;  // a phase appends at most one candidate per allowed row
    bool overflow = false;
    CS_TRY(w->read_overflow(w->stream, &overflow));
    if (!overflow) return CS_OK;
    sc->overflow_reruns.fetch_add(1);
    CS_HIP(hipMemsetAsync(w->bs.d_overflow, 0, 2 * sizeof(uint32_t), w->stream));  // (run_scoped: the overflow is the scope's alone)
    return similar_list_scan(h, sc, w, plan, nq, k, gv, sv, keys);
}

// The similar-chunk searches (scan_similar.hip): the sources resolved on the host (similar_sources.hpp), their rows gathered
// into w->d_queries on the device, the scan's arithmetic under the per-query exclusions, the ordinary merge.  Over the whole
// store (scope_given false: run_similar — the streaming scan over every stored row, or the filter with the similar refine) or
// over a scope's row list (run_similar_scoped: the gathered scan, or the int8 filter planned over the scope's rows, by the
// scope's route).  Every check, the scope's handle-level ones before the ids, comes before the scope's list is
// refreshed; groups_mu is released before the scope's mutex is taken.
int32_t search_similar(cs_index* h, bool scope_given, cs_scope* scope, const uint32_t* ids, uint32_t nq, uint32_t k,
                       int32_t exclude, float min_cos, const HostAnswer& out) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    CS_TRY(check_search(h, nq, h->dim, k));
    if (!ids || !out.cos || !out.ids || !out.counts) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (!similar_mode_ok(exclude))
        return fail(CS_ERR_BAD_ARG, "exclude must be CS_SIMILAR_EXCLUDE_NONE, _SELF or _GROUP (0..2), got %d", exclude);
    if (min_cos != min_cos) return fail(CS_ERR_BAD_ARG, "min_cos is NaN");
    if (scope_given) CS_TRY(check_scope_handle(h, scope));
    DeviceGuard g(h->device);
    GroupView gv{nullptr, 0, h->ledger.id_base(), 0xFFFFFFFFu};
    {
        std::lock_guard<std::mutex> lk(h->groups_mu);  // (ensure_groups below moves the table's upload marks under it)
        const SourceCheck sc = resolve_similar_sources(h->ledger, h->groups, ids, nq, exclude, nullptr, nullptr, nullptr);
        if (sc.fault == SourceFault::NeverIssued)
            return fail(CS_ERR_BAD_ARG, "ids[%u] = %u was never issued (the index has issued ids %u to %llu)", sc.at, ids[sc.at],
                        h->ledger.id_base(), (unsigned long long)h->ledger.next_id());
        if (sc.fault == SourceFault::Deleted)
            return fail(CS_ERR_BAD_ARG, "ids[%u] = %u: the chunk was deleted", sc.at, ids[sc.at]);
    }
    uint64_t rows = h->ledger.stored();
    ScopedFilterPlan fp;
    if (scope_given) {
        CS_TRY(scope_ready(h, scope, &rows, &fp, nq, k));
        if (rows == 0) return empty_answer(nq, k, out);  // nothing of the scope is stored
    }
    if (exclude == CS_SIMILAR_EXCLUDE_GROUP) CS_TRY(ensure_groups(h, 0xFFFFFFFFu, &gv));
    const ScanPlan plan = plan_scan(rows, h->dim, nq, k, h->num_cus);  // a scope: the grid follows the list's length
    return host_search(h, nullptr, nq, k, plan.partial_keys, plan.merge_keys, out, [&](Workspace* w, uint64_t* keys) {
        CS_TRY(w->reserve_similar(nq));
        {
            std::lock_guard<std::mutex> lk(h->groups_mu);
            resolve_similar_sources(h->ledger, h->groups, ids, nq, exclude, w->h_similar, w->h_similar + nq, w->h_similar + 2 * (size_t)nq);
        }
        CS_HIP(hipMemcpyAsync(w->d_similar, w->h_similar, 3 * (size_t)nq * sizeof(uint32_t), hipMemcpyHostToDevice, w->stream));
        CS_TRY(launch_gather_sources(h->d_corpus, h->dim, w->d_similar, nq, w->d_queries, w->stream));
        const SimilarView sv{w->d_similar + nq, w->d_similar + 2 * (size_t)nq, min_cos};
        if (scope_given) return run_similar_scoped(h, scope, w, plan, rows, fp, nq, k, gv, sv, keys);
        return run_similar(h, w, plan, nq, k, gv, sv, keys);
    });
}

}  // namespace

extern "C" {

const char* cs_last_error(void) { return last_error_ref().c_str(); }
uint32_t cs_abi_version(void) { return 6; }  // 5: cs_bert_config gained arch, rotary_base; 6: rotary_base_local, local_window, global_every

int32_t cs_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int32_t cs_index_create(uint32_t dim, uint64_t capacity_rows, int32_t device, uint32_t id_base,
                        cs_index** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (dim == 0 || dim > 8192) return fail(CS_ERR_BAD_ARG, "dim must be in 1..8192, got %u", dim);
    int ndev = 0;
    CS_HIP(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev)
        return fail(CS_ERR_HIP, "HIP device %d not available (%d visible); there is no CPU fallback",
                    device, ndev);
    DeviceGuard g(device);
    hipDeviceProp_t prop;
    CS_HIP(hipGetDeviceProperties(&prop, device));
    cs_index* h = new cs_index();
    h->device = device;
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->dim = dim;
    h->ledger = IndexLedger(id_base);
    {
        const char* env = std::getenv("CS_INDEX_SPLIT");  // "0": keep the batched path on the exact-f32 MFMA
        h->use_split = split_scan_supported(dim) && !(env && env[0] == '0');
        const char* e8 = std::getenv("CS_FILTER_INT8");  // "0": filter on the f16 copy only
        h->use_q8 = h->use_split && !(e8 && e8[0] == '0');
        const char* ee = std::getenv("CS_FILTER_F16_EAGER");  // "1": keep the f16 copy beside a serving int8 copy
        h->f16_eager = (ee && ee[0] == '1') || cs_lab_env("CS_FILTER_INT8_MAX_Q") != nullptr;
        if (const char* e = std::getenv("CS_FILTER_INT8_MAX_SPREAD")) h->q8_max_spread = (float)std::atof(e);
        if (const char* e = std::getenv("CS_INDEX_COMPACT_DEAD_PCT")) h->compact_dead_pct = (uint32_t)std::max(0, std::min(100, std::atoi(e)));
    }
    h->route = route_knobs_from_env();
    if (const char* e = std::getenv("CS_SIMILAR_ROUTE"))  // auto | scan | filter (anything else: auto)
        h->similar_route.store(!strcmp(e, "scan") ? CS_SIMILAR_ROUTE_SCAN : !strcmp(e, "filter") ? CS_SIMILAR_ROUTE_FILTER : CS_SIMILAR_ROUTE_AUTO);
    if (h->use_split) {
        // does the f16 MFMA take subnormal inputs exactly?  One one-wave launch per device per process.
        static std::mutex mu;
        static std::map<int, bool> known;
        std::lock_guard<std::mutex> lk(mu);
        auto it = known.find(device);
        if (it == known.end()) {
            bool ok = false;
            int32_t s = sh_denorm_selftest(&ok, nullptr);
            if (s != CS_OK) { delete h; return s; }
            it = known.emplace(device, ok).first;
        }
        h->filter_margin = filter_margin(dim, it->second);
    }
    if (capacity_rows) {
        int32_t s = grow(h, capacity_rows);
        if (s != CS_OK) { delete h; return s; }
    }
    *out = h;
    return CS_OK;
}

void cs_index_destroy(cs_index* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    (void)drain_appends(h);
    for (auto* w : h->pool) { w->release_all(); delete w; }
    for (auto& kv : h->by_stream) { kv.second->release_all(); delete kv.second; }
    free_join_pools(h);
    for (auto& t : h->pending) {
        (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); (void)hipEventDestroy(t.e2);
    }
    if (h->d_corpus) (void)hipFree(h->d_corpus);
    if (h->d_dead) (void)hipFree(h->d_dead);
    if (h->d_norms) (void)hipFree(h->d_norms);
    if (h->d_split) (void)hipFree(h->d_split);
    if (h->d_q8) (void)hipFree(h->d_q8);
    if (h->d_tmeta) (void)hipFree(h->d_tmeta);
    if (h->d_mu) (void)hipFree(h->d_mu);
    if (h->d_ids) (void)hipFree(h->d_ids);
    if (h->d_groups) (void)hipFree(h->d_groups);
    if (h->d_classes) (void)hipFree(h->d_classes);
    delete h;
}

int32_t cs_index_add(cs_index* h, const float* rows, uint64_t n, uint32_t dim, uint32_t* out_ids) {
    CS_TRY(check_append(h, n, dim));
    if (n == 0) return CS_OK;  // store.rs:655-657
    if (!rows) return fail(CS_ERR_BAD_ARG, "rows is null");
    DeviceGuard g(h->device);
    CS_TRY(grow(h, h->ledger.stored() + n));
    CS_HIP(hipMemcpy(h->d_corpus + (size_t)h->ledger.stored() * h->dim, rows,
                     (size_t)n * h->dim * sizeof(float), hipMemcpyHostToDevice));
    finish_append(h, n, out_ids);
    return CS_OK;
}

int32_t cs_index_add_device(cs_index* h, const float* d_rows, uint64_t n, uint32_t dim,
                            uint32_t* out_ids, void* stream) {
    CS_TRY(check_append(h, n, dim));
    if (n == 0) return CS_OK;
    if (!d_rows) return fail(CS_ERR_BAD_ARG, "d_rows is null");
    DeviceGuard g(h->device);
    CS_TRY(grow(h, h->ledger.stored() + n));
    CS_HIP(hipMemcpyAsync(h->d_corpus + (size_t)h->ledger.stored() * h->dim, d_rows,
                          (size_t)n * h->dim * sizeof(float), hipMemcpyDeviceToDevice,
                          (hipStream_t)stream));
    finish_append(h, n, out_ids);
    return CS_OK;
}

// E8 in place ("optionally write straight into corpus matrix row"): room for n more rows is made, *d_rows is where
// they go — the caller has them WRITTEN there (cs_embedder_embed_*_device with this address as its output: the pooling kernel's
// own stores land in the corpus) — and cs_index_commit_rows makes them rows of the index with the next n ids.  No staging buffer,
// no device-to-device copy.  Between the two calls the handle must see no other mutating call (&mut self, as insert_chunks).
int32_t cs_index_reserve_rows(cs_index* h, uint64_t n, uint32_t dim, float** d_rows) {
    CS_TRY(check_append(h, n, dim));
    if (!d_rows) return fail(CS_ERR_BAD_ARG, "d_rows is null");
    DeviceGuard g(h->device);
    CS_TRY(grow(h, h->ledger.stored() + n));
    *d_rows = h->d_corpus + (size_t)h->ledger.stored() * h->dim;
    return CS_OK;
}

int32_t cs_index_commit_rows(cs_index* h, uint64_t n, uint32_t* out_ids) {
    CS_TRY(check_append(h, n, h ? h->dim : 0));
    if (h->ledger.stored() + n > h->capacity)
        return fail(CS_ERR_BAD_ARG, "cs_index_commit_rows: %llu rows were not reserved (capacity %llu, stored %llu)", (unsigned long long)n,
                    (unsigned long long)h->capacity, (unsigned long long)h->ledger.stored());
    finish_append(h, n, out_ids);
    return CS_OK;
}

int32_t cs_index_add_synthetic(cs_index* h, uint64_t n, uint64_t seed, uint64_t first_row,
                               uint32_t* out_first_id) {
    CS_TRY(check_append(h, n, h ? h->dim : 0));
    DeviceGuard g(h->device);
    CS_TRY(grow(h, h->ledger.stored() + n));
    CS_TRY(launch_synth_fill(h->d_corpus + (size_t)h->ledger.stored() * h->dim, n, h->dim, seed, first_row,
                             nullptr));
    CS_HIP(hipStreamSynchronize(nullptr));
    if (out_first_id) *out_first_id = h->ledger.next_id();
    finish_append(h, n, nullptr);
    return CS_OK;
}

int32_t cs_index_remove(cs_index* h, const uint32_t* ids, uint64_t n, uint64_t* removed) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (removed) *removed = 0;
    if (n == 0) return CS_OK;  // store.rs:585-587
    if (!ids) return fail(CS_ERR_BAD_ARG, "ids is null");
    const uint64_t cnt = h->ledger.remove(ids, n);
    if (cnt) {
        h->built = false;  // store.rs:604-606
        DeviceGuard g(h->device);
        const std::vector<uint32_t>& dead = h->ledger.dead_words();
        CS_HIP(hipMemcpy(h->d_dead, dead.data(), dead.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (removed) *removed = cnt;
    return CS_OK;
}

int32_t cs_index_build(cs_index* h) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    CS_TRY(drain_appends(h));  // appended rows (incl. async device appends) are now visible
    if (h->ledger.wants_reclaim(h->compact_dead_pct)) CS_TRY(compact(h));
    if (h->ledger.compacted() && h->ids_uploaded < h->ledger.stored()) {  // the row -> id table of a compacted index, for the rows that are new
        if (h->ids_cap < h->ledger.stored()) {
            uint32_t* nt = nullptr;
            const uint64_t cap = std::max<uint64_t>(h->capacity, h->ledger.stored());
            CS_HIP(hipMalloc(&nt, (size_t)cap * sizeof(uint32_t)));
            if (h->d_ids) (void)hipFree(h->d_ids);
            h->d_ids = nt;
            h->ids_cap = cap;
            h->ids_uploaded = 0;
        }
        CS_HIP(hipMemcpy(h->d_ids + h->ids_uploaded, h->ledger.ids_data() + h->ids_uploaded,
                         (size_t)(h->ledger.stored() - h->ids_uploaded) * sizeof(uint32_t), hipMemcpyHostToDevice));
        h->ids_uploaded = h->ledger.stored();
    }
    if ((batched_supported(h->dim) || h->use_split) && h->normed_rows < h->ledger.stored()) {
        CS_TRY(launch_row_norms(h->d_corpus, h->normed_rows, h->ledger.stored() - h->normed_rows, h->dim,
                                h->d_norms, nullptr));
        CS_HIP(hipDeviceSynchronize());
        h->normed_rows = h->ledger.stored();
    }
    if (h->use_q8 && h->d_q8 && h->q8_rows / 128 < h->ledger.stored() / 128) {  // tiles that became complete
        if (!h->d_mu) CS_HIP(hipMalloc(&h->d_mu, h->dim * sizeof(float)));
        if (h->q8_rows == 0)  // first tiles of this copy: centre it on the mean unit row of what is there now
            CS_TRY(launch_unit_mean(h->d_corpus, h->d_norms, std::min<uint64_t>(h->ledger.stored(), 1u << 20), h->dim, h->d_mu, nullptr));
        CS_TRY(launch_corpus_q8(h->d_corpus, h->d_norms, h->d_q8, h->d_tmeta, h->q8_rows / 128,
                                h->ledger.stored() / 128 - h->q8_rows / 128, h->dim, h->d_mu, nullptr));
        CS_HIP(hipDeviceSynchronize());
        h->q8_rows = h->ledger.stored() / 128 * 128;
        // outlier coordinates: the tile scale is the tile's largest |u - mu|; where the typical tile's is far above what
        // evenly spread coordinates give (4.3 / sqrt(dim) for Gaussian rows), the band (it grows with the square) lets
        // through more rows than the candidate buffers hold — the f16 copy serves the filter then
        {
            const uint64_t nt = std::min<uint64_t>(h->q8_rows / 128, 4096);
            std::vector<float4> tm((size_t)nt);
            CS_HIP(hipMemcpy(tm.data(), h->d_tmeta, (size_t)nt * sizeof(float4), hipMemcpyDeviceToHost));
            std::vector<float> sp;
            sp.reserve((size_t)nt);
            for (const float4& t : tm)
                if (t.x == t.x && t.x > 0.0f) sp.push_back(127.0f / t.x * std::sqrt((float)h->dim));
            if (!sp.empty()) {
                std::nth_element(sp.begin(), sp.begin() + sp.size() / 2, sp.end());
                h->q8_spread = sp[sp.size() / 2];
                if (h->q8_spread > h->q8_max_spread) h->q8_active.store(false);
            }
        }
    }
    if (h->use_split) {
        // The f16 copy is kept only where the int8 copy does not serve (none, retired, <= 1024 rows) or on request: an
        // index the int8 copy serves holds f32 + int8 = 5 bytes per element and its builds skip the conversion pass.
        // Should the int8 copy be retired later (two overflowed searches), the first search after that builds it.
        if (h->f16_eager || !q8_serves(h)) {
            (void)ensure_f16(h);  // no room: not an error — searches take the exact paths
        } else if (h->d_split) {
            std::lock_guard<std::mutex> lk(h->filter_mu);
            (void)hipFree(h->d_split);
            h->d_split = nullptr;
            h->split_rows = 0;
            h->split_cap = 0;
        }
    }
    h->build_gen.fetch_add(1);       // scopes remake their row lists
    h->built = true;                 // store.rs:428
    return CS_OK;
}

int32_t cs_index_clear(cs_index* h) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    CS_TRY(drain_appends(h));
    if (h->d_dead && h->capacity)
        CS_HIP(hipMemset(h->d_dead, 0, (size_t)((h->capacity + 31) / 32) * sizeof(uint32_t)));
    h->ledger.clear();  // store.rs:701 next_id = 0: ids restart at id_base, the identity numbering again
    h->ids_uploaded = 0;
    h->normed_rows = 0;
    h->split_rows = 0;
    h->f16_failed = false;
    h->q8_rows = 0;
    h->q8_active.store(true);
    h->q8_strikes.store(0);
    h->q8_searches.store(0);
    {  // the groups go with the ids (the device table keeps its room)
        std::lock_guard<std::mutex> lk(h->groups_mu);
        h->groups.clear();
    }
    {  // and so do the classes, with their device table (the device is idle: drain_appends synchronised it)
        std::lock_guard<std::mutex> lk(h->classes_mu);
        h->classes.clear();
        h->classes_cap = 0;
        CS_HIP(realloc_buf(h->d_classes, 0));
    }
    h->build_gen.fetch_add(1);
    h->built = false;  // store.rs:702
    return CS_OK;
}

int32_t cs_index_is_built(const cs_index* h) { return h && h->built ? 1 : 0; }
uint64_t cs_index_len(const cs_index* h) { return h ? h->ledger.live() : 0; }
uint64_t cs_index_stored_rows(const cs_index* h) { return h ? h->ledger.stored() : 0; }
uint32_t cs_index_next_id(const cs_index* h) { return h ? h->ledger.next_id() : 0; }
uint32_t cs_index_dim(const cs_index* h) { return h ? h->dim : 0; }
int32_t cs_index_device(const cs_index* h) { return h ? h->device : -1; }

int32_t cs_index_search(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                        float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_all(h, queries, nq, dim, k, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_device(cs_index* h, const float* d_queries, uint32_t nq, uint32_t dim,
                               uint32_t k, uint64_t* d_out_keys, float* d_out_cos,
                               uint32_t* d_out_ids, uint32_t* d_out_counts, void* stream) {
    CS_TRY(check_search(h, nq, dim, k));
    if (!d_queries) return fail(CS_ERR_BAD_ARG, "d_queries is null");
    DeviceGuard g(h->device);
    const ScanPlan plan = plan_scan(h->ledger.stored(), h->dim, nq, k, h->num_cus);
    Workspace* w = for_stream(h, (hipStream_t)stream);
    CS_TRY(w->reserve(plan.partial_keys, plan.merge_keys, nq, h->dim, k, false));
    return run_search(h, w, plan, d_queries, nq, k, d_out_keys, d_out_cos, d_out_ids, d_out_counts,
                      (hipStream_t)stream, nullptr, /*may_sync=*/false);
}

int32_t cs_index_search_variants(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                 float* out_cos, uint32_t* out_ids, uint32_t* out_count,
                                 int32_t* out_high_confidence) {
    return search_all(h, queries, nq, dim, k, HostAnswer{out_cos, out_ids, out_count, out_high_confidence, true});
}

int32_t cs_index_search_masked(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                               const uint32_t* allow, uint64_t allow_bits, float* out_cos, uint32_t* out_ids,
                               uint32_t* out_counts) {
    return search_masked(h, queries, nq, dim, k, allow, allow_bits, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_variants_masked(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                        const uint32_t* allow, uint64_t allow_bits, float* out_cos, uint32_t* out_ids,
                                        uint32_t* out_count, int32_t* out_high_confidence) {
    return search_masked(h, queries, nq, dim, k, allow, allow_bits,
                         HostAnswer{out_cos, out_ids, out_count, out_high_confidence, true});
}

int32_t cs_index_set_groups(cs_index* h, const uint32_t* ids, const uint32_t* groups, uint64_t n) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (n == 0) return CS_OK;
    if (!ids || !groups) return fail(CS_ERR_BAD_ARG, "ids or groups is null");
    std::lock_guard<std::mutex> lk(h->groups_mu);
    const int64_t bad = h->groups.set(ids, groups, n, h->ledger);
    if (bad >= 0)
        return fail(CS_ERR_BAD_ARG, "ids[%llu] = %u was never issued (the index has issued ids %u to %llu)",
                    (unsigned long long)bad, ids[bad], h->ledger.id_base(), (unsigned long long)h->ledger.next_id());
    return CS_OK;
}

int32_t cs_index_groups_info(cs_index* h, uint64_t* assigned_ids, uint64_t* table_bytes) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    std::lock_guard<std::mutex> lk(h->groups_mu);
    if (assigned_ids) *assigned_ids = h->groups.assigned();
    if (table_bytes) *table_bytes = h->groups_cap * sizeof(uint32_t);
    return CS_OK;
}

int32_t cs_index_set_classes(cs_index* h, const uint32_t* ids, const uint16_t* classes, uint64_t n) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (n == 0) return CS_OK;
    if (!ids || !classes) return fail(CS_ERR_BAD_ARG, "ids or classes is null");
    std::lock_guard<std::mutex> lk(h->classes_mu);
    const int64_t bad = h->classes.set(ids, classes, n, h->ledger);
    if (bad >= 0)
        return fail(CS_ERR_BAD_ARG, "ids[%llu] = %u was never issued (the index has issued ids %u to %llu)",
                    (unsigned long long)bad, ids[bad], h->ledger.id_base(), (unsigned long long)h->ledger.next_id());
    return CS_OK;
}

int32_t cs_index_classes_info(cs_index* h, uint64_t* assigned_ids, uint64_t* table_bytes) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    std::lock_guard<std::mutex> lk(h->classes_mu);
    if (assigned_ids) *assigned_ids = h->classes.assigned();
    if (table_bytes) *table_bytes = h->classes_cap * sizeof(uint16_t);
    return CS_OK;
}

int32_t cs_index_search_boosted(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, const float* weights,
                                uint32_t n_classes, float* out_score, float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_boosted(h, false, nullptr, queries, nq, dim, k, weights, n_classes, out_score, out_cos, out_ids, out_counts);
}

int32_t cs_index_search_grouped(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k, uint32_t per_group,
                                float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_grouped(h, false, nullptr, queries, nq, dim, k, per_group, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_variants_grouped(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                         uint32_t per_group, float* out_cos, uint32_t* out_ids, uint32_t* out_count,
                                         int32_t* out_high_confidence) {
    return search_grouped(h, false, nullptr, queries, nq, dim, k, per_group,
                          HostAnswer{out_cos, out_ids, out_count, out_high_confidence, true});
}

int32_t cs_index_search_similar(cs_index* h, const uint32_t* ids, uint32_t nq, uint32_t k, int32_t exclude, float min_cos,
                                float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_similar(h, false, nullptr, ids, nq, k, exclude, min_cos, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_similar_scoped(cs_index* h, cs_scope* scope, const uint32_t* ids, uint32_t nq, uint32_t k,
                                       int32_t exclude, float min_cos, float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_similar(h, true, scope, ids, nq, k, exclude, min_cos, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_scope_create(cs_index* h, const uint32_t* ids, uint64_t n, cs_scope** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    CS_TRY(check_scope_ids(ids, n));
    DeviceGuard g(h->device);
    cs_scope* sc = new_index_scope(h);
    const int32_t st = [&]() -> int32_t {
        CS_TRY(scope_alloc(h, sc, n));
        if (n) {
            CS_HIP(hipMemcpyAsync(sc->d_ids, ids, (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice, sc->stream));
            CS_HIP(hipStreamSynchronize(sc->stream));  // `ids` is the caller's again
        }
        return scope_first_list(h, sc);
    }();
    if (st != CS_OK) {
        scope_free(sc);
        return st;
    }
    *out = sc;
    return CS_OK;
}

int32_t cs_index_scope_create_range(cs_index* h, uint32_t first_id, uint64_t n, cs_scope** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    CS_TRY(check_scope_range(first_id, n));
    DeviceGuard g(h->device);
    cs_scope* sc = new_index_scope(h);
    const int32_t st = [&]() -> int32_t {
        CS_TRY(scope_alloc(h, sc, n));
        if (n) {
            CS_TRY(launch_scope_range(first_id, n, sc->d_ids, sc->stream));
            CS_HIP(hipStreamSynchronize(sc->stream));
        }
        return scope_first_list(h, sc);
    }();
    if (st != CS_OK) {
        scope_free(sc);
        return st;
    }
    *out = sc;
    return CS_OK;
}

int32_t cs_scope_combine(const cs_scope* a, const cs_scope* b, int32_t op, cs_scope** out) {
    if (!out) return fail(CS_ERR_BAD_ARG, "out is null");
    *out = nullptr;
    if (!a) return fail(CS_ERR_BAD_ARG, "null scope handle (a)");
    if (!b) return fail(CS_ERR_BAD_ARG, "null scope handle (b)");
    if (op != CS_SCOPE_OP_UNION && op != CS_SCOPE_OP_INTERSECT && op != CS_SCOPE_OP_DIFFERENCE)
        return fail(CS_ERR_BAD_ARG, "op must be CS_SCOPE_OP_UNION, _INTERSECT or _DIFFERENCE, got %d", op);
    if ((a->index != nullptr) != (b->index != nullptr))
        return fail(CS_ERR_BAD_ARG, "the scopes were made for different stores: one over an index, one over a sharded store");
    if (a->index != b->index || a->shards != b->shards || a->parts.size() != b->parts.size())
        return fail(CS_ERR_BAD_ARG, "the scopes were made for different stores");
    if (a->index) return scope_combine_one(a, b, op, out);
    // sharded: the stripe map sends one global id to one shard, so the per-shard operations are the global one
    cs_scope* sc = new cs_scope();
    sc->shards = a->shards;
    uint64_t total = 0;
    for (size_t s = 0; s < a->parts.size(); ++s) {
        cs_scope* part = nullptr;
        int32_t st = scope_combine_one(a->parts[s], b->parts[s], op, &part);
        if (st == CS_OK) {
            sc->parts.push_back(part);
            total += part->n_ids;
            if (total > 0xffffffffull) st = fail(CS_ERR_BAD_ARG, "a scope holds at most 2^32 - 1 ids (ids are u32): the union names every id");
        }
        if (st != CS_OK) {
            scope_free(sc);
            return st;
        }
    }
    *out = sc;
    return CS_OK;
}

int32_t cs_scope_read_ids(const cs_scope* scope, uint64_t first, uint64_t n, uint32_t* out_ids) {
    if (!scope) return fail(CS_ERR_BAD_ARG, "null scope handle");
    uint64_t have = scope->n_ids;
    for (const cs_scope* p : scope->parts) have += p->n_ids;  // (n_ids never changes after the scope was made)
    if (first > have || n > have - first)
        return fail(CS_ERR_BAD_ARG, "ids [%llu, %llu) asked of a scope of %llu ids", (unsigned long long)first,
                    (unsigned long long)(first + n), (unsigned long long)have);
    if (n == 0) return CS_OK;
    if (!out_ids) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (!scope->index) return shards_scope_read_ids(scope, first, n, out_ids);
    return scope_part_read_ids(scope, first, n, out_ids);
}

uint32_t cs_scope_ops_tile(void) { return kScopeOpsTile; }

void cs_scope_destroy(cs_scope* scope) {
    if (scope) scope_free(scope);
}

int32_t cs_scope_info(const cs_scope* scope, uint64_t* n_ids, uint64_t* live_rows, uint64_t* refreshes) {
    if (!scope) return fail(CS_ERR_BAD_ARG, "null scope handle");
    uint64_t n = 0, live = 0, made = 0;
    auto one = [&](const cs_scope* sc) {
        std::lock_guard<std::mutex> lk(sc->mu);
        n += sc->n_ids;
        live += sc->live_rows;
        made = std::max(made, sc->refreshes);
    };
    if (scope->index) one(scope);
    for (const cs_scope* p : scope->parts) one(p);
    if (n_ids) *n_ids = n;
    if (live_rows) *live_rows = live;
    if (refreshes) *refreshes = made;
    return CS_OK;
}

int32_t cs_scope_set_route(cs_scope* scope, int32_t route) {
    if (!scope) return fail(CS_ERR_BAD_ARG, "null scope handle");
    if (!scope->index) return fail(CS_ERR_BAD_ARG, "a scope over a sharded store always takes the gathered scan");
    if (route != CS_SCOPE_ROUTE_AUTO && route != CS_SCOPE_ROUTE_GATHER && route != CS_SCOPE_ROUTE_FILTER)
        return fail(CS_ERR_BAD_ARG, "route must be CS_SCOPE_ROUTE_AUTO, _GATHER or _FILTER, got %d", route);
    scope->route.store(route);
    return CS_OK;
}

int32_t cs_scope_route_info(const cs_scope* scope, uint64_t* filter_searches, uint64_t* gathered_searches,
                            uint64_t* overflow_reruns, uint64_t* extra_bytes) {
    if (!scope) return fail(CS_ERR_BAD_ARG, "null scope handle");
    uint64_t extra = 0;
    if (scope->index) {
        std::lock_guard<std::mutex> lk(scope->mu);
        extra = (uint64_t)(scope->blocked_words + scope->table_words) * sizeof(uint32_t);
    }
    uint64_t filter = scope->filter_searches.load(), gathered = scope->gathered_searches.load(), reruns = scope->overflow_reruns.load();
    for (const cs_scope* part : scope->parts) {  // a sharded scope: what its parts counted (a grouped search counts one per part)
        filter += part->filter_searches.load();
        gathered += part->gathered_searches.load();
        reruns += part->overflow_reruns.load();
    }
    if (filter_searches) *filter_searches = filter;
    if (gathered_searches) *gathered_searches = gathered;
    if (overflow_reruns) *overflow_reruns = reruns;
    if (extra_bytes) *extra_bytes = extra;
    return CS_OK;
}

int32_t cs_index_search_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                               float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_scoped(h, scope, queries, nq, dim, k, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_variants_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim,
                                        uint32_t k, float* out_cos, uint32_t* out_ids, uint32_t* out_count,
                                        int32_t* out_high_confidence) {
    return search_scoped(h, scope, queries, nq, dim, k, HostAnswer{out_cos, out_ids, out_count, out_high_confidence, true});
}

int32_t cs_index_search_grouped_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                       uint32_t per_group, float* out_cos, uint32_t* out_ids, uint32_t* out_counts) {
    return search_grouped(h, true, scope, queries, nq, dim, k, per_group, HostAnswer{out_cos, out_ids, out_counts, nullptr, false});
}

int32_t cs_index_search_boosted_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                       const float* weights, uint32_t n_classes, float* out_score, float* out_cos,
                                       uint32_t* out_ids, uint32_t* out_counts) {
    return search_boosted(h, true, scope, queries, nq, dim, k, weights, n_classes, out_score, out_cos, out_ids, out_counts);
}

int32_t cs_index_search_variants_boosted(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                         const float* weights, uint32_t n_classes, float* out_score, float* out_cos,
                                         uint32_t* out_ids, uint32_t* out_count, int32_t* out_high_confidence) {
    return search_variants_boosted(h, false, nullptr, nullptr, queries, nq, dim, k, weights, n_classes, out_score, out_cos, out_ids,
                                   out_count, out_high_confidence);
}

int32_t cs_index_search_variants_boosted_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim,
                                                uint32_t k, const float* weights, uint32_t n_classes, float* out_score,
                                                float* out_cos, uint32_t* out_ids, uint32_t* out_count,
                                                int32_t* out_high_confidence) {
    return search_variants_boosted(h, true, scope, nullptr, queries, nq, dim, k, weights, n_classes, out_score, out_cos, out_ids,
                                   out_count, out_high_confidence);
}

int32_t cs_index_search_variants_boosted_grouped(cs_index* h, const float* queries, uint32_t nq, uint32_t dim, uint32_t k,
                                                 uint32_t per_group, const float* weights, uint32_t n_classes, float* out_score,
                                                 float* out_cos, uint32_t* out_ids, uint32_t* out_count,
                                                 int32_t* out_high_confidence) {
    return search_variants_boosted(h, false, nullptr, &per_group, queries, nq, dim, k, weights, n_classes, out_score, out_cos,
                                   out_ids, out_count, out_high_confidence);
}

int32_t cs_index_search_variants_boosted_grouped_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq,
                                                        uint32_t dim, uint32_t k, uint32_t per_group, const float* weights,
                                                        uint32_t n_classes, float* out_score, float* out_cos, uint32_t* out_ids,
                                                        uint32_t* out_count, int32_t* out_high_confidence) {
    return search_variants_boosted(h, true, scope, &per_group, queries, nq, dim, k, weights, n_classes, out_score, out_cos,
                                   out_ids, out_count, out_high_confidence);
}

int32_t cs_index_search_variants_grouped_scoped(cs_index* h, cs_scope* scope, const float* queries, uint32_t nq, uint32_t dim,
                                                uint32_t k, uint32_t per_group, float* out_cos, uint32_t* out_ids,
                                                uint32_t* out_count, int32_t* out_high_confidence) {
    return search_grouped(h, true, scope, queries, nq, dim, k, per_group,
                          HostAnswer{out_cos, out_ids, out_count, out_high_confidence, true});
}

int32_t cs_index_search_scoped_device(cs_index* h, cs_scope* scope, const float* d_queries, uint32_t nq, uint32_t dim,
                                      uint32_t k, uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                                      uint32_t* d_out_counts, void* stream) {
    CS_TRY(check_search(h, nq, dim, k));
    if (!d_queries) return fail(CS_ERR_BAD_ARG, "d_queries is null");
    DeviceGuard g(h->device);
    uint64_t live = 0;
    CS_TRY(scope_ready(h, scope, &live));  // (waits for the device only when the list has to be remade)
    hipStream_t st = (hipStream_t)stream;
    if (live == 0) {  // the empty answer, enqueued: keys 0, cosines 0, ids 0xFFFFFFFF, counts 0
        const size_t on = (size_t)nq * k;
        if (d_out_keys) CS_HIP(hipMemsetAsync(d_out_keys, 0, on * sizeof(uint64_t), st));
        if (d_out_cos) CS_HIP(hipMemsetAsync(d_out_cos, 0, on * sizeof(float), st));
        if (d_out_ids) CS_HIP(hipMemsetAsync(d_out_ids, 0xFF, on * sizeof(uint32_t), st));
        if (d_out_counts) CS_HIP(hipMemsetAsync(d_out_counts, 0, (size_t)nq * sizeof(uint32_t), st));
        return CS_OK;
    }
    const ScanPlan plan = plan_scan(live, h->dim, nq, k, h->num_cus);
    Workspace* w = for_stream(h, st);
    CS_TRY(w->reserve(plan.partial_keys, plan.merge_keys, nq, h->dim, k, false));
    return run_row_list(h, w, plan, live, scope->d_list, scope->d_blocks + scope_list_blocks(scope->n_ids), d_queries, nq, k,
                        d_out_keys, d_out_cos, d_out_ids, d_out_counts, st);
}

int32_t cs_merge_variants_device(int32_t device, const uint64_t* d_keys, uint32_t nv, uint32_t k, uint32_t limit,
                                 uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_count,
                                 uint32_t* d_out_high_confidence, void* stream) {
    if (!d_keys || nv == 0 || nv > CS_MAX_VARIANTS || k == 0 || k > CS_MAX_K || limit == 0 || limit > CS_MAX_K)
        return fail(CS_ERR_BAD_ARG, "bad variant-merge arguments");
    DeviceGuard g(device);
    return launch_merge_variants(d_keys, nv, k, limit, d_out_keys, d_out_cos, d_out_ids, d_out_count,
                                 d_out_high_confidence, (hipStream_t)stream);
}

int32_t cs_index_search_status(cs_index* h, void* stream, uint32_t* overflowed) {
    if (!h || !overflowed) return fail(CS_ERR_BAD_ARG, "null argument");
    *overflowed = 0;
    DeviceGuard g(h->device);
    Workspace* w = nullptr;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        auto it = h->by_stream.find(std::make_pair((hipStream_t)stream, std::this_thread::get_id()));
        if (it != h->by_stream.end()) w = it->second;
    }
    if (!w || !w->bs.d_overflow) return CS_OK;  // no batched search was issued here
    CS_HIP(hipMemcpyAsync(w->h_overflow, w->bs.d_overflow, 3 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                          (hipStream_t)stream));
    CS_HIP(hipMemsetAsync(w->bs.d_overflow + 1, 0, sizeof(uint32_t), (hipStream_t)stream));
    CS_HIP(hipStreamSynchronize((hipStream_t)stream));
    *overflowed = w->h_overflow[1];
    return CS_OK;
}

int32_t cs_index_release_stream(cs_index* h, void* stream) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    std::vector<Workspace*> gone;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        for (auto it = h->by_stream.begin(); it != h->by_stream.end();) {
            if (it->first.first == (hipStream_t)stream) { gone.push_back(it->second); it = h->by_stream.erase(it); }
            else ++it;
        }
    }
    if (gone.empty()) return CS_OK;
    CS_HIP(hipStreamSynchronize((hipStream_t)stream));  // searches still using the scratch
    uint64_t fallbacks = 0;
    for (Workspace* w : gone) {
        if (w->bs.d_overflow) {  // overflows counted on the device so far stay in the handle's totals
            uint32_t v[3] = {0, 0, 0};
            CS_HIP(hipMemcpy(v, w->bs.d_overflow, sizeof v, hipMemcpyDeviceToHost));
            fallbacks += (uint64_t)v[2] + (v[0] ? 1 : 0);
        }
        w->release_all();
        delete w;
    }
    cs::merge_scratch_release(h->device, (hipStream_t)stream);
    std::lock_guard<std::mutex> lk(h->mu);
    h->batched_fallbacks += fallbacks;
    return CS_OK;
}

int32_t cs_merge_topk_device(int32_t device, const uint64_t* d_keys, uint32_t nlists, uint32_t nq,
                             uint32_t k, uint64_t* d_out_keys, float* d_out_cos,
                             uint32_t* d_out_ids, uint32_t* d_out_counts, void* stream) {
    return cs::merge_topk_device_impl(device, d_keys, nlists, nq, k, d_out_keys, d_out_cos, d_out_ids, d_out_counts,
                                      (hipStream_t)stream, 0, 0);
}

}  // extern "C"

namespace {
struct MergeScratch { uint64_t* a = nullptr; uint64_t* b = nullptr; size_t cap = 0; };
std::mutex g_merge_mu;
std::map<std::tuple<int, hipStream_t, std::thread::id>, MergeScratch> g_merge_pool;
}  // namespace

// the caller has synchronised `stream`
void cs::merge_scratch_release(int device, hipStream_t stream) {
    std::lock_guard<std::mutex> lk(g_merge_mu);
    for (auto it = g_merge_pool.begin(); it != g_merge_pool.end();) {
        if (std::get<0>(it->first) == device && std::get<1>(it->first) == stream) {
            if (it->second.a) { (void)hipFree(it->second.a); (void)hipFree(it->second.b); }
            it = g_merge_pool.erase(it);
        } else ++it;
    }
}

int32_t cs::index_search_masked_device(cs_index* h, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* allow,
                                       uint64_t allow_bits, uint64_t* d_out_keys, hipStream_t stream) {
    CS_TRY(check_search(h, nq, h ? h->dim : 0, k));
    if (!d_queries || !d_out_keys) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (!allow && allow_bits) return fail(CS_ERR_BAD_ARG, "allow is null");
    DeviceGuard g(h->device);
    const uint64_t bound = masked_bound(h, allow, allow_bits);
    if (bound == 0) {  // empty lists for the merge behind
        CS_HIP(hipMemsetAsync(d_out_keys, 0, (size_t)nq * k * sizeof(uint64_t), stream));
        return CS_OK;
    }
    const ScanPlan plan = plan_scan(bound, h->dim, nq, k, h->num_cus);
    Workspace* w = for_stream(h, stream);
    CS_TRY(w->reserve(plan.partial_keys, plan.merge_keys, nq, h->dim, k, false));
    return run_masked(h, w, plan, bound, d_queries, nq, k, allow, allow_bits, d_out_keys, stream);
}

// search_grouped's two kinds with the queries in HBM and the keys to a device pointer (scan.hpp): the same plan, scan and
// merge, on the caller's stream.
int32_t cs::index_search_grouped_device(cs_index* h, cs_scope* scope, const float* d_queries, uint32_t nq, uint32_t k,
                                        uint32_t per_group, uint64_t* d_out_keys, hipStream_t stream) {
    CS_TRY(check_search(h, nq, h ? h->dim : 0, k));
    if (!d_queries || !d_out_keys) return fail(CS_ERR_BAD_ARG, "null buffer");
    if (per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    DeviceGuard g(h->device);
    uint64_t rows = h->ledger.stored();
    if (scope) CS_TRY(scope_ready(h, scope, &rows));
    if (rows == 0) {  // empty lists for the merge behind: the gather slot may hold an earlier search's keys
        CS_HIP(hipMemsetAsync(d_out_keys, 0, (size_t)nq * k * sizeof(uint64_t), stream));
        return CS_OK;
    }
    GroupView gv;
    CS_TRY(ensure_groups(h, per_group, &gv));
    const GroupedPlan plan = plan_grouped(rows, h->dim, nq, k, h->num_cus);  // a scope: the grid follows the list's length
    Workspace* w = for_stream(h, stream);
    CS_TRY(w->reserve(plan.partial_keys, plan.merge_keys, nq, h->dim, k, false));
    if (!scope) return run_grouped(h, w, plan, gv, d_queries, nq, k, d_out_keys, stream);
    scope->gathered_searches.fetch_add(1);
    return run_grouped_list(h, w, plan, gv, scope->d_list, scope->d_blocks + scope_list_blocks(scope->n_ids), d_queries, nq, k,
                            d_out_keys, stream);
}

int32_t cs::index_scope_live_rows(cs_index* h, cs_scope* scope, uint64_t* live_rows) {
    if (!h || !h->built) return fail(CS_ERR_NOT_BUILT, "Index not built. Call build_index() after inserting chunks.");
    DeviceGuard g(h->device);
    return scope_ready(h, scope, live_rows);
}

int32_t cs::index_reserve(cs_index* h, uint64_t rows) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    return grow(h, rows);
}

int32_t cs::index_append_from(cs_index* h, const float* d_rows, int src_device, uint64_t n, hipStream_t stream) {
    CS_TRY(check_append(h, n, h ? h->dim : 0));
    if (n == 0) return CS_OK;
    {
        DeviceGuard g(h->device);
        CS_TRY(grow(h, h->ledger.stored() + n));
    }
    float* dst = h->d_corpus + (size_t)h->ledger.stored() * h->dim;
    const size_t bytes = (size_t)n * h->dim * sizeof(float);
    DeviceGuard g(src_device);  // `stream` belongs to the source device
    if (src_device == h->device) CS_HIP(hipMemcpyAsync(dst, d_rows, bytes, hipMemcpyDeviceToDevice, stream));
    else {
        CS_HIP(hipMemcpyPeerAsync(dst, h->device, d_rows, src_device, bytes, stream));
        cs_index::ForeignAppend* slot = nullptr;
        for (auto& fe : h->foreign_appends)
            if (fe.device == src_device && fe.stream == stream) { slot = &fe; break; }
        if (slot) {  // the same stream again: re-recording its event covers this copy and every earlier one
            if (hipEventRecord(slot->done, stream) != hipSuccess) return fail(CS_ERR_HIP, "hipEventRecord on the peer stream failed");
        } else {
            hipEvent_t done = nullptr;
            CS_HIP(hipEventCreateWithFlags(&done, hipEventDisableTiming));
            if (hipEventRecord(done, stream) != hipSuccess) {
                (void)hipEventDestroy(done);
                return fail(CS_ERR_HIP, "hipEventRecord on the peer stream failed");
            }
            h->foreign_appends.push_back({src_device, stream, done});
        }
    }
    finish_append(h, n, nullptr);
    return CS_OK;
}

int32_t cs::merge_topk_device_impl(int32_t device, const uint64_t* d_keys, uint32_t nlists, uint32_t nq, uint32_t k,
                                   uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_counts,
                                   hipStream_t stream, uint32_t remap_stripe, uint32_t remap_shards) {
    if (!d_keys || nlists == 0 || nq == 0 || k == 0 || k > CS_MAX_K)
        return fail(CS_ERR_BAD_ARG, "bad merge arguments");
    DeviceGuard g(device);
    const size_t tmp = merge_tmp_keys(nlists, nq, k);
    uint64_t *ta = nullptr, *tb = nullptr;
    if (tmp) {
        // More than one merge level (over 2048 keys per query; 8 shards x k <= 256 fit one): ping-pong scratch
        // kept per (device, stream, calling thread) and grown on demand — never freed or synchronised per call, so
        // the merge stays asynchronous between the all-gather and whatever the caller enqueues next.
        std::lock_guard<std::mutex> lk(g_merge_mu);
        MergeScratch& sc = g_merge_pool[std::make_tuple(device, (hipStream_t)stream, std::this_thread::get_id())];
        if (tmp > sc.cap) {
            // the old pair may still be in use by merges already enqueued on this stream: let them finish
            if (sc.a) { CS_HIP(hipStreamSynchronize((hipStream_t)stream)); (void)hipFree(sc.a); (void)hipFree(sc.b); }
            sc = MergeScratch();
            CS_HIP(hipMalloc(&sc.a, tmp * sizeof(uint64_t)));
            CS_HIP(hipMalloc(&sc.b, tmp * sizeof(uint64_t)));
            sc.cap = tmp;
        }
        ta = sc.a;
        tb = sc.b;
    }
    return launch_merge(d_keys, nlists, nq, k, true, ta, tb, d_out_keys, d_out_cos, d_out_ids, d_out_counts,
                        (hipStream_t)stream, nullptr, remap_stripe, remap_shards);
}

extern "C" {

int32_t cs_index_read_rows(cs_index* h, uint64_t first_row, uint64_t n, float* out_rows) {
    if (!h || !out_rows) return fail(CS_ERR_BAD_ARG, "null argument");
    if (first_row + n > h->ledger.issued_ids())
        return fail(CS_ERR_BAD_ARG, "rows [%llu, %llu) out of range (have %llu)",
                    (unsigned long long)first_row, (unsigned long long)(first_row + n),
                    (unsigned long long)h->ledger.issued_ids());
    if (n == 0) return CS_OK;
    DeviceGuard g(h->device);
    CS_TRY(drain_appends(h));
    // rows are named by their ids (first_row = id - id_base): runs of neighbours in one copy (all of them, until a reclaim)
    for (uint64_t i = 0; i < n;) {
        const IndexLedger::Run run = h->ledger.id_run(first_row + i, n - i);
        if (run.row == kNoRow)
            return fail(CS_ERR_BAD_ARG, "row of id %u was deleted and reclaimed by cs_index_build",
                        h->ledger.id_base() + (uint32_t)(first_row + i));
        CS_HIP(hipMemcpy(out_rows + (size_t)i * h->dim, h->d_corpus + (size_t)run.row * h->dim,
                         (size_t)run.len * h->dim * sizeof(float), hipMemcpyDeviceToHost));
        i += run.len;
    }
    return CS_OK;
}

int32_t cs_index_set_filter_min_queries(cs_index* h, uint32_t min_queries) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    h->route.filter_min_q = min_queries < 1 ? 1 : (int)min_queries;
    return CS_OK;
}

int32_t cs_index_set_single_query_route(cs_index* h, int32_t route) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (route != CS_ROUTE_COST && route != CS_ROUTE_STREAM && route != CS_ROUTE_FILTER)
        return fail(CS_ERR_BAD_ARG, "route must be CS_ROUTE_COST, CS_ROUTE_STREAM or CS_ROUTE_FILTER, got %d", route);
    h->route.single_route = route;
    return CS_OK;
}

int32_t cs_index_set_similar_route(cs_index* h, int32_t route) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (route != CS_SIMILAR_ROUTE_AUTO && route != CS_SIMILAR_ROUTE_SCAN && route != CS_SIMILAR_ROUTE_FILTER)
        return fail(CS_ERR_BAD_ARG, "route must be CS_SIMILAR_ROUTE_AUTO, _SCAN or _FILTER (0..2), got %d", route);
    h->similar_route.store(route);
    return CS_OK;
}

int32_t cs_index_similar_route_info(cs_index* h, uint64_t* filter_searches, uint64_t* scan_searches, uint64_t* filter_fallbacks) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    if (filter_searches) *filter_searches = h->similar_filter_searches.load();
    if (scan_searches) *scan_searches = h->similar_scan_searches.load();
    if (filter_fallbacks) *filter_fallbacks = h->similar_filter_fallbacks.load();
    return CS_OK;
}

int32_t cs_index_debug_counters(cs_index* h, uint64_t* batched_searches, uint64_t* batched_fallbacks) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    // device-API searches count their overflows on the device (no host round trip per search): drain and read
    uint64_t dev_fallbacks = 0;
    std::vector<Workspace*> ws;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        for (auto& kv : h->by_stream) ws.push_back(kv.second);
    }
    for (Workspace* w : ws) {
        if (!w->bs.d_overflow) continue;
        uint32_t v[3] = {0, 0, 0};
        // a caller's stream may have been destroyed since (cs_index_release_stream is the orderly way): the blocking
        // copy below orders against everything still running on the device either way
        if (hipStreamSynchronize(w->stream) != hipSuccess) (void)hipGetLastError();
        CS_HIP(hipMemcpy(v, w->bs.d_overflow, sizeof v, hipMemcpyDeviceToHost));
        dev_fallbacks += (uint64_t)v[2] + (v[0] ? 1 : 0);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    if (batched_searches) *batched_searches = h->batched_searches;
    if (batched_fallbacks) *batched_fallbacks = h->batched_fallbacks + dev_fallbacks;
    return CS_OK;
}

int32_t cs_index_filter_state(cs_index* h, int32_t* copy, float* spread, uint64_t* int8_reruns) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    std::lock_guard<std::mutex> lk(h->mu);
    const bool i8 = q8_serves(h);
    if (copy) *copy = i8 ? 2 : h->use_split ? 1 : 0;
    if (spread) *spread = h->q8_spread;
    if (int8_reruns) *int8_reruns = h->q8_reruns;
    return CS_OK;
}

int32_t cs_index_filter_copies(cs_index* h, int32_t* has_int8, int32_t* has_f16, uint64_t* filter_bytes) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    std::lock_guard<std::mutex> lk(h->filter_mu);
    const bool i8 = h->d_q8 && h->q8_rows > 0, f16 = h->d_split && h->split_rows > 0;
    if (has_int8) *has_int8 = i8 ? 1 : 0;
    if (has_f16) *has_f16 = f16 ? 1 : 0;
    if (filter_bytes)
        *filter_bytes = (h->d_q8 ? ((uint64_t)h->capacity + 255) / 256 * 256 * h->dim : 0) +
                        (h->d_split ? (uint64_t)h->split_cap * h->dim * 2 : 0);
    return CS_OK;
}

int32_t cs_index_profile(cs_index* h, int32_t enable) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->profile = enable != 0;
    return CS_OK;
}

int32_t cs_index_profile_read(cs_index* h, double* scan_ms, uint64_t* scan_launches,
                              double* merge_ms, int32_t reset) {
    if (!h) return fail(CS_ERR_BAD_ARG, "null index handle");
    DeviceGuard g(h->device);
    std::vector<EventTriple> pend;
    {
        std::lock_guard<std::mutex> lk(h->mu);
        pend.swap(h->pending);
    }
    double s_ms = 0.0, m_ms = 0.0;
    for (auto& t : pend) {
        CS_HIP(hipEventSynchronize(t.e2));
        float a = 0.f, b = 0.f;
        CS_HIP(hipEventElapsedTime(&a, t.e0, t.e1));
        CS_HIP(hipEventElapsedTime(&b, t.e1, t.e2));
        s_ms += a;
        m_ms += b;
        (void)hipEventDestroy(t.e0); (void)hipEventDestroy(t.e1); (void)hipEventDestroy(t.e2);
    }
    std::lock_guard<std::mutex> lk(h->mu);
    h->scan_ms += s_ms;
    h->merge_ms += m_ms;
    h->scan_launches += pend.size();
    if (scan_ms) *scan_ms = h->scan_ms;
    if (merge_ms) *merge_ms = h->merge_ms;
    if (scan_launches) *scan_launches = h->scan_launches;
    if (reset) { h->scan_ms = 0.0; h->merge_ms = 0.0; h->scan_launches = 0; }
    return CS_OK;
}

}  // extern "C"
