// scan_similar.hip — the similar-chunk search: the exact best k live rows for a query that IS a stored row, without the
// rows the caller excludes (the source chunk itself; every chunk of its group, its file).  A caller without it reads the
// row back, searches with it and filters the ranked list on the host: the chunk finds itself first and its own file next,
// and a file of near-duplicates fills the list before anything from another file appears.  The exclusion
// therefore happens inside the selection, as the cap of the grouped search does (scan_grouped.hip).
// Host side: similar_sources.hpp resolves source ids to rows and per-query exclusions; index.hip search_similar enqueues.
//
//   1. gather: the nq source rows, corpus -> the workspace's query buffer, verbatim: gather_sources_kernel.  The query
//      rows never leave HBM.
//   2. scan: scan_topk_kernel's tile loop (scan.hip), a row scored by the functions that score it there (scan_wave.hpp:
//      load_query_fragment, row_products, cosine_of — so every cosine is bit-identical).  No gate word, no prime pass.
//      Every list starts from floor = min_cos, so the fast-path test `c > thr` rejects rows under the bound from the first
//      tile on.  On the slow path a row that beats the threshold and is alive is compared with the query's excluded id
//      and, when the query has an excluded group, its group (one table read per wave) with that; an excluded row is never
//      inserted.  The queries of one tile carry different exclusions.
//   3. merge: a wave's list holds only rows the answer may contain, so no level needs a cap: the block merge
//      (block_merge_store) and the ordinary launch_merge finish it, on plan_scan's geometry.
//   4. inside a scope (cs_index_search_similar_scoped): step 2 over the scope's row list instead of every stored row —
//      the gathered scan's tile loop (scan_masked.hip part 2) with this file's list state and slow path: the end of the
//      kernels below.  Steps 1 and 3 are the same.
#include "scan.hpp"
#include "grouped_plan.hpp"  // kNoGroup
#include "scan_wave.hpp"

namespace cs {

static_assert(kNoGroup == CS_NO_GROUP, "grouped_plan.hpp restates the public constant");

// scan_grouped.hip's, restated: the group of an id under the table as the kernels read it
__device__ __forceinline__ uint32_t similar_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;  // ids past the table (appended after the last assignment) are ungrouped
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

// May query (ex_id, ex_group) return the row that carries `id`?  ex_id = an id no row carries: nothing excluded by id;
// ex_group = CS_NO_GROUP: nothing excluded by group (an ungrouped row is never excluded by group).
__device__ __forceinline__ bool similar_keeps(const GroupView& gv, uint32_t id, uint32_t ex_id, uint32_t ex_group) {
    if (id == ex_id) return false;
    return ex_group == kNoGroup || similar_group_of(gv, id) != ex_group;
}

// ---- 1. gather ------------------------------------------------------------------------------------------
// Block q copies stored row rows[q] to queries[q].  dim is a multiple of 4 for the tuned dims only: plain floats.
__global__ void __launch_bounds__(kBlock)
gather_sources_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows, uint32_t dim,
                      float* __restrict__ queries) {
    const uint32_t q = blockIdx.x;
    const float* src = corpus + (size_t)rows[q] * dim;
    float* dst = queries + (size_t)q * dim;
    for (uint32_t c = threadIdx.x; c < dim; c += kBlock) dst[c] = src[c];
}

// ---- 2. scan ----------------------------------------------------------------------------------------------
// scan_topk_kernel (scan.hip) without PRIME and the gate: see there for J, U and QT.  ex_ids / ex_groups: [nq].
template <int J, int U, int QT>
__global__ void __launch_bounds__(kBlock)
scan_similar_topk_kernel(const float* __restrict__ corpus, uint64_t n_rows, const float* __restrict__ queries, uint32_t nq,
                         uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds id_base, GroupView gv,
                         const uint32_t* __restrict__ ex_ids, const uint32_t* __restrict__ ex_groups, float min_cos,
                         uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad]
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
    float thr[QT], floor[QT];
    uint32_t wpos[QT], ex_id[QT], ex_group[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        const uint32_t q = (q0 + qi < nq) ? (q0 + qi) : (nq - 1);
        qmag[qi] = load_query_fragment<J>(queries, q, l32, qf[qi]);
        ex_id[qi] = ex_ids[q];
        ex_group[qi] = ex_groups[q];
        floor[qi] = min_cos;
        thr[qi] = floor[qi];
        wpos[qi] = 0;
    }
    __syncthreads();

    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const uint64_t ntiles = (n_rows + 2 * U - 1) / (2 * U);

    for (uint64_t tile = gw; tile < ntiles; tile += nw) {
        const uint64_t row0 = tile * (2 * U);
        f32x4 x[U][J];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint64_t r = row0 + 2 * u + half;
            r = r < n_rows ? r : n_rows - 1;  // tail rows re-read the last row, masked below
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + r * DIM) + l32;
#pragma unroll
            for (int j = 0; j < J; ++j) x[u][j] = __builtin_nontemporal_load(p + j * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot[QT];
            const float xmag = row_products<J, QT>(x[u], qf, dot);
            const uint64_t r = row0 + 2 * u + half;
            const bool valid = r < n_rows;
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                const float d = half_allreduce_sum(dot[qi]);
                const float c = cosine_of(d, qmag[qi], xmag);
                unsigned long long m = __ballot(valid && l32 == 0 && c > thr[qi]);
                if (m) {  // rare: wave-uniform slow path (the rows of an excluded file all come here and leave one by one)
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float cc = __shfl(c, src, 64);
                        const uint64_t rr = row0 + 2 * u + (src >> 5);
                        if (cc > thr[qi] && !row_is_dead(dead, rr)) {
                            const uint32_t id = id_base.of(rr);
                            if (similar_keeps(gv, id, ex_id[qi], ex_group[qi]))
                                wave_list_insert(list, k, lane, cc, id, thr[qi], wpos[qi], floor[qi]);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();

    // block merge: the 4 wave lists of each query -> best k, sorted, to HBM
    const uint32_t nsort = kWaves * kpad;
#pragma unroll 1
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= nq) break;
        block_merge_store(lds_keys + (size_t)qi * nsort, kpad, k, q0 + qi, tid, partial);
    }
}

// Any other dim: one wave per row, lanes stride over columns (wave_row_cosine, scan_wave.hpp).
__global__ void __launch_bounds__(kBlock)
scan_similar_generic_kernel(const float* __restrict__ corpus, uint64_t n_rows, uint32_t dim, const float* __restrict__ queries,
                            uint32_t nq, uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds id_base,
                            GroupView gv, const uint32_t* __restrict__ ex_ids, const uint32_t* __restrict__ ex_groups,
                            float min_cos, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    const uint32_t ex_id = ex_ids[q], ex_group = ex_groups[q];
    float thr = min_cos;
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = gw; r < n_rows; r += nw) {
        const float* xp = corpus + r * dim;
        const float c = wave_row_cosine(xp, qp, dim, lane, qmag);
        if (c > thr && !row_is_dead(dead, r)) {  // wave-uniform
            const uint32_t id = id_base.of(r);
            if (similar_keeps(gv, id, ex_id, ex_group)) wave_list_insert(list, k, lane, c, id, thr, wpos, min_cos);
        }
    }
    __syncthreads();
    block_merge_store(lds_keys, kpad, k, q, tid, partial);
}

// ---- 4. scan over a scope's row list ------------------------------------------------------------------------
// scan_masked_topk_kernel's tile loop (scan_masked.hip part 2, not its prime pass) under scan_similar_topk_kernel's list
// state and slow path: half-wave h of tile t scores row rows[t * 2U + 2u + h] of the list rows[0, *rows_len).  The list
// holds live rows only (launch_scope_rows), in ascending row order, so there is no tombstone read and a wave still meets
// its rows in ascending id.  A row that beats the threshold resolves its id, is tested against the query's exclusions and
// only then inserted.
//
// Registers: plan_scan sizes the grid to be fully resident from the streaming scan's occupancy, and at 384-d with four queries
// per pass that is three blocks per CU: 168 VGPRs.  The unscoped kernel has 167 and the masked scan 168; this one came out
// at 169, which the allocation granule of 8 turns into two blocks per CU and a grid with a second round of blocks (DESIGN.md
// §8d).  That shape alone therefore declares the three waves per SIMD it is launched for; every other shape is launched at
// one or two blocks per CU and fits as it is.
template <int J, int QT>
constexpr int similar_list_waves_per_simd() { return (J == 3 && QT == 4) ? 3 : 1; }

template <int J, int U, int QT>
__global__ void __launch_bounds__(kBlock, (similar_list_waves_per_simd<J, QT>()))
scan_similar_list_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                         const uint32_t* __restrict__ rows_len, const float* __restrict__ queries, uint32_t nq, uint32_t k,
                         uint32_t kpad, RowIds row_ids, GroupView gv, const uint32_t* __restrict__ ex_ids,
                         const uint32_t* __restrict__ ex_groups, float min_cos, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad]
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;
    const uint64_t n_list = *rows_len;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
    float thr[QT], floor[QT];
    uint32_t wpos[QT], ex_id[QT], ex_group[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        const uint32_t q = (q0 + qi < nq) ? (q0 + qi) : (nq - 1);
        qmag[qi] = load_query_fragment<J>(queries, q, l32, qf[qi]);
        ex_id[qi] = ex_ids[q];
        ex_group[qi] = ex_groups[q];
        floor[qi] = min_cos;
        thr[qi] = floor[qi];
        wpos[qi] = 0;
    }
    __syncthreads();

    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const uint64_t ntiles = (n_list + 2 * U - 1) / (2 * U);

    for (uint64_t tile = gw; tile < ntiles; tile += nw) {
        const uint64_t e0 = tile * (2 * U);  // list entries of this tile
        f32x4 x[U][J];
        uint32_t row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint64_t e = e0 + 2 * u + half;
            e = e < n_list ? e : n_list - 1;  // tail entries re-read the last entry, masked below
            row[u] = rows[e];
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + (uint64_t)row[u] * DIM) + l32;
#pragma unroll
            for (int j = 0; j < J; ++j) x[u][j] = __builtin_nontemporal_load(p + j * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot[QT];
            const float xmag = row_products<J, QT>(x[u], qf, dot);
            const bool valid = e0 + 2 * u + half < n_list;
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                const float d = half_allreduce_sum(dot[qi]);
                const float c = cosine_of(d, qmag[qi], xmag);
                unsigned long long m = __ballot(valid && l32 == 0 && c > thr[qi]);
                if (m) {  // rare: wave-uniform slow path; half 0 (the lower list entry) first
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float cc = __shfl(c, src, 64);
                        const uint32_t rr = __shfl(row[u], src, 64);
                        if (cc > thr[qi]) {
                            const uint32_t id = row_ids.of(rr);
                            if (similar_keeps(gv, id, ex_id[qi], ex_group[qi]))
                                wave_list_insert(list, k, lane, cc, id, thr[qi], wpos[qi], floor[qi]);
                        }
                    }
                }
            }
        }
    }
    __syncthreads();

    const uint32_t nsort = kWaves * kpad;
#pragma unroll 1
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= nq) break;
        block_merge_store(lds_keys + (size_t)qi * nsort, kpad, k, q0 + qi, tid, partial);
    }
}

// Any other dim: one wave per list entry, lanes stride over columns (wave_row_cosine, scan_wave.hpp).  A template only to
// be emitted with the instantiations, behind every kernel this file already had: their labels keep their numbers, so their
// device code stays the same text (benchmarks/compare_device_code.py).
template <int = 0>
__global__ void __launch_bounds__(kBlock)
scan_similar_list_generic_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                                 const uint32_t* __restrict__ rows_len, uint32_t dim, const float* __restrict__ queries,
                                 uint32_t nq, uint32_t k, uint32_t kpad, RowIds row_ids, GroupView gv,
                                 const uint32_t* __restrict__ ex_ids, const uint32_t* __restrict__ ex_groups, float min_cos,
                                 uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    const uint64_t n_list = *rows_len;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    const uint32_t ex_id = ex_ids[q], ex_group = ex_groups[q];
    float thr = min_cos;
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t e = gw; e < n_list; e += nw) {
        const uint32_t r = rows[e];
        const float* xp = corpus + (uint64_t)r * dim;
        const float c = wave_row_cosine(xp, qp, dim, lane, qmag);
        if (c > thr) {  // wave-uniform
            const uint32_t id = row_ids.of(r);
            if (similar_keeps(gv, id, ex_id, ex_group)) wave_list_insert(list, k, lane, c, id, thr, wpos, min_cos);
        }
    }
    __syncthreads();
    block_merge_store(lds_keys, kpad, k, q, tid, partial);
}

// ---- host side ------------------------------------------------------------------------------------------

int32_t launch_gather_sources(const float* d_corpus, uint32_t dim, const uint32_t* d_rows, uint32_t nq, float* d_queries,
                              hipStream_t stream) {
    if (nq == 0) return CS_OK;
    hipLaunchKernelGGL(gather_sources_kernel, dim3(nq), dim3(kBlock), 0, stream, d_corpus, d_rows, dim, d_queries);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

template <int J, int U, int QT>
static void launch_similar_fast(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, const float* d_queries,
                                uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv,
                                const SimilarView& sv, uint64_t* d_partial, hipStream_t stream) {
    const size_t lds = (size_t)QT * kWaves * plan.kpad * sizeof(uint64_t);
    hipLaunchKernelGGL((scan_similar_topk_kernel<J, U, QT>), dim3(plan.blocks, plan.passes), dim3(kBlock), lds, stream,
                       d_corpus, n_rows, d_queries, nq, k, plan.kpad, d_dead, ids, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos,
                       d_partial);
}

template <int J, int U>
static void launch_similar_q(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, const float* d_queries, uint32_t nq,
                             uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv, const SimilarView& sv,
                             uint64_t* d_partial, hipStream_t stream) {
    switch (plan.qtile) {
        case 4: launch_similar_fast<J, U, 4>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream); break;
        case 2: launch_similar_fast<J, U, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream); break;
        default: launch_similar_fast<J, U, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream); break;
    }
}

int32_t launch_scan_similar(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries,
                            uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv,
                            const SimilarView& sv, uint64_t* d_partial, hipStream_t stream) {
    if (!sv.d_ex_ids || !sv.d_ex_groups || sv.min_cos != sv.min_cos)
        return fail(CS_ERR_BAD_ARG, "similar scan needs its exclusion arrays and a bound that is a number");
    if (plan.kpad < k || plan.qtile < 1 || (size_t)plan.qtile * kWaves * plan.kpad * sizeof(uint64_t) > 64 * 1024)
        return fail(CS_ERR_BAD_ARG, "similar scan plan does not fit: qtile %u, kpad %u for k %u", plan.qtile, plan.kpad, k);
    if (n_rows == 0) {  // nothing to score: all-empty partial lists
        CS_HIP(hipMemsetAsync(d_partial, 0, plan.partial_keys * sizeof(uint64_t), stream));
        return CS_OK;
    }
    const bool fast = dim == 384 || dim == 768 || dim == 1024;
    if (fast && plan.deep && plan.qtile == 1) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_similar_fast<3, 8, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
        else if (dim == 768) launch_similar_fast<6, 4, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
        else launch_similar_fast<8, 3, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
    } else if (dim == 384) launch_similar_q<3, 4>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
    else if (dim == 768) launch_similar_q<6, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
    else if (dim == 1024) launch_similar_q<8, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, sv, d_partial, stream);
    else {
        const size_t lds = (size_t)kWaves * plan.kpad * sizeof(uint64_t);
        hipLaunchKernelGGL(scan_similar_generic_kernel, dim3(plan.blocks, nq), dim3(kBlock), lds, stream, d_corpus, n_rows, dim,
                           d_queries, nq, k, plan.kpad, d_dead, ids, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos, d_partial);
    }
    CS_HIP(hipGetLastError());
    return CS_OK;
}

template <int J, int U, int QT>
static void launch_similar_list_fast(const ScanPlan& plan, const float* d_corpus, const uint32_t* d_list, const uint32_t* d_len,
                                     const float* d_queries, uint32_t nq, uint32_t k, RowIds ids, const GroupView& gv,
                                     const SimilarView& sv, uint64_t* d_partial, hipStream_t stream) {
    const size_t lds = (size_t)QT * kWaves * plan.kpad * sizeof(uint64_t);
    hipLaunchKernelGGL((scan_similar_list_kernel<J, U, QT>), dim3(plan.blocks, plan.passes), dim3(kBlock), lds, stream,
                       d_corpus, d_list, d_len, d_queries, nq, k, plan.kpad, ids, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos,
                       d_partial);
}

template <int J, int U>
static void launch_similar_list_q(const ScanPlan& plan, const float* d_corpus, const uint32_t* d_list, const uint32_t* d_len,
                                  const float* d_queries, uint32_t nq, uint32_t k, RowIds ids, const GroupView& gv,
                                  const SimilarView& sv, uint64_t* d_partial, hipStream_t stream) {
    switch (plan.qtile) {
        case 4: launch_similar_list_fast<J, U, 4>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, sv, d_partial, stream); break;
        case 2: launch_similar_list_fast<J, U, 2>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, sv, d_partial, stream); break;
        default: launch_similar_list_fast<J, U, 1>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, sv, d_partial, stream); break;
    }
}

int32_t launch_scan_similar_list(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const GroupView& gv, const SimilarView& sv, uint64_t* d_partial, hipStream_t stream) {
    if (!sv.d_ex_ids || !sv.d_ex_groups || sv.min_cos != sv.min_cos)
        return fail(CS_ERR_BAD_ARG, "similar scan needs its exclusion arrays and a bound that is a number");
    if (!d_list || !d_list_len) return fail(CS_ERR_BAD_ARG, "similar scan over a row list needs the list and its length");
    if (plan.kpad < k || plan.qtile < 1 || (size_t)plan.qtile * kWaves * plan.kpad * sizeof(uint64_t) > 64 * 1024)
        return fail(CS_ERR_BAD_ARG, "similar scan plan does not fit: qtile %u, kpad %u for k %u", plan.qtile, plan.kpad, k);
    const bool fast = dim == 384 || dim == 768 || dim == 1024;
    if (fast && plan.deep && plan.qtile == 1) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_similar_list_fast<3, 8, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
        else if (dim == 768) launch_similar_list_fast<6, 4, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
        else launch_similar_list_fast<8, 3, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
    } else if (dim == 384) launch_similar_list_q<3, 4>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
    else if (dim == 768) launch_similar_list_q<6, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
    else if (dim == 1024) launch_similar_list_q<8, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, sv, d_partial, stream);
    else {
        const size_t lds = (size_t)kWaves * plan.kpad * sizeof(uint64_t);
        hipLaunchKernelGGL(scan_similar_list_generic_kernel<>, dim3(plan.blocks, nq), dim3(kBlock), lds, stream, d_corpus, d_list,
                           d_list_len, dim, d_queries, nq, k, plan.kpad, ids, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos,
                           d_partial);
    }
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
