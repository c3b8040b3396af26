// scan_boosted_grouped.hip — the boosted search under the per-file cap: the exact best k live rows by b = fl(score(cosine) *
// weight of the row's class) such that no group contributes more than per_group of them, and the cosines of the winners
// of a boosted search over query variants.  The reference does all of it in one search, each step on the list the step
// before left: up to nine variants merged, the kind and language boosts on the hits already ranked, `--per-file` on the
// re-sorted list (src/search/mod.rs).  Contract: include/codesearch_gpu.h, cs_index_search_variants_boosted; why capped
// lists of b may be merged, and in levels: grouped_plan.hpp; DESIGN.md §8g.
//
//   1. boosted capped scan: scan_boosted_topk_kernel's tile loop (scan_boosted.hip) — the same scoring functions, the
//      same pre-gate boosted_bound(s, wmin, wmax) > thr that rejects most rows without reading a class — with the capped
//      wave list of scan_grouped.hip beside it: a u32 group slot per key slot.  A row past the pre-gate reads its class
//      and weight and forms b; only if b > thr does it read its group and take wave_list_insert_grouped with b as the
//      value.  thr is the list's worst b once the list is full and -inf before: a full list whose worst key the row does
//      not beat holds k cap-valid rows that all beat it.  Rows arrive by ascending id, so packed keys settle ties.
//      LIST: over a scope's row list, as the gathered scans read it; else every stored row with the tombstone test.
//      No prime pass (under a cap the k-th largest wave maximum does not bound the capped k-th: grouped_plan.hpp) and no
//      block merge (an uncapped level): each wave's list goes to HBM and launch_merge_grouped, which orders keys of any
//      float, finishes every variant.
//   2. cosine of the winners across variants: the merged keys carry b and the id.  boosted_variants_cos_kernel is
//      boosted_cos_kernel with a loop over the nq variants: it scores the winner's row against each with the same
//      functions and writes the largest cosine — the c of which b is the boosted score, since score and rounding are
//      monotone.
#include "scan.hpp"
#include "grouped_plan.hpp"
#include "scan_wave.hpp"
#include "scan_rules.hpp"

namespace cs {

// ---- 1. boosted capped scan ------------------------------------------------------------------------------
// See scan_topk_kernel (scan.hip) for J, U and QT.  LIST: half-wave h of tile t takes row rows[t * 2U + 2u + h] of
// rows[0, *rows_len) (live rows only, ascending: no tombstone read); else row t * 2U + 2u + h of [0, n_rows).
template <int J, int U, int QT, bool LIST>
__global__ void __launch_bounds__(kBlock)
scan_boosted_grouped_topk_kernel(const float* __restrict__ corpus, uint64_t n_rows, const uint32_t* __restrict__ rows,
                                 const uint32_t* __restrict__ rows_len, const float* __restrict__ queries, uint32_t nq,
                                 uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds row_ids, BoostView bv,
                                 GroupView gv, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)QT * kWaves * kpad);
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;
    const uint64_t n = LIST ? (uint64_t)*rows_len : n_rows;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
    float thr[QT];
    uint32_t wpos[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        qmag[qi] = load_query_fragment<J>(queries, (q0 + qi < nq) ? (q0 + qi) : (nq - 1), l32, qf[qi]);
        thr[qi] = -__builtin_huge_valf();
        wpos[qi] = 0;
    }
    const float wmin = bv.wmin, wmax = bv.wmax;
    __syncthreads();

    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    const uint64_t ntiles = (n + 2 * U - 1) / (2 * U);

    for (uint64_t tile = gw; tile < ntiles; tile += nw) {
        const uint64_t e0 = tile * (2 * U);  // rows (LIST: list entries) of this tile
        f32x4 x[U][J];
        uint32_t row[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            uint64_t e = e0 + 2 * u + half;
            e = e < n ? e : n - 1;  // the tail re-reads the last row, masked below
            const uint64_t r = LIST ? (uint64_t)rows[e] : e;
            row[u] = (uint32_t)r;  // read on the slow path by LIST only
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + r * DIM) + l32;
#pragma unroll
            for (int j = 0; j < J; ++j) x[u][j] = __builtin_nontemporal_load(p + j * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot[QT];
            const float xmag = row_products<J, QT>(x[u], qf, dot);
            const bool valid = e0 + 2 * u + half < n;
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                const float d = half_allreduce_sum(dot[qi]);
                const float s = boosted_score(cosine_of(d, qmag[qi], xmag));
                unsigned long long m = __ballot(valid && l32 == 0 && boosted_bound(s, wmin, wmax) > thr[qi]);  // the pre-gate: no class read
                if (m) {  // wave-uniform slow path; half 0 (the lower row, the lower id) first
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    volatile uint32_t* glist = lds_groups + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float ss = __shfl(s, src, 64);
                        const uint64_t rr = LIST ? (uint64_t)__shfl(row[u], src, 64) : e0 + 2 * u + (src >> 5);
                        if (boosted_bound(ss, wmin, wmax) > thr[qi] && (LIST || !row_is_dead(dead, rr))) {
                            const uint32_t id = row_ids.of(rr);
                            const float b = ss * boosted_weight(bv, id);
                            if (b > thr[qi])  // only now the group
                                wave_list_insert_grouped(list, glist, k, gv.per_group, lane, b, id, group_of(gv, id), thr[qi],
                                                         wpos[qi]);
                        }
                    }
                }
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= nq) break;
        wave_list_store(lds_keys + ((size_t)qi * kWaves + wave) * kpad, k, lane, partial, q0 + qi, wave);
    }
}

// Any other dim: one wave per row (LIST: per list entry), lanes stride over columns (wave_row_cosine, scan_wave.hpp).
template <bool LIST>
__global__ void __launch_bounds__(kBlock)
scan_boosted_grouped_generic_kernel(const float* __restrict__ corpus, uint64_t n_rows, const uint32_t* __restrict__ rows,
                                    const uint32_t* __restrict__ rows_len, uint32_t dim, const float* __restrict__ queries,
                                    uint32_t nq, uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds row_ids,
                                    BoostView bv, GroupView gv, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)kWaves * kpad);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    const uint64_t n = LIST ? (uint64_t)*rows_len : n_rows;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    const float wmin = bv.wmin, wmax = bv.wmax;
    float thr = -__builtin_huge_valf();
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    volatile uint32_t* glist = lds_groups + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t e = gw; e < n; e += nw) {
        const uint64_t r = LIST ? (uint64_t)rows[e] : e;
        const float s = boosted_score(wave_row_cosine(corpus + r * dim, qp, dim, lane, qmag));
        if (boosted_bound(s, wmin, wmax) > thr && (LIST || !row_is_dead(dead, r))) {  // wave-uniform
            const uint32_t id = row_ids.of(r);
            const float b = s * boosted_weight(bv, id);
            if (b > thr) wave_list_insert_grouped(list, glist, k, gv.per_group, lane, b, id, group_of(gv, id), thr, wpos);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    wave_list_store(lds_keys + (size_t)wave * kpad, k, lane, partial, q, wave);
}

// ---- 2. cosine of the winners across variants ---------------------------------------------------------------
// Wave (blockIdx.x * kWaves + wave) takes winner j of the ONE merged list keys[k]: out_cos[j] = the largest over the nv
// variants of the streaming scan's cosine of the winner's row (0 for an empty slot), out_keys[j] = the key (optional).
// J = dim / 128 for the tuned dims — both half-waves score the row, as either would in the scan — and 0 for any other dim.
template <int J>
__global__ void __launch_bounds__(kBlock)
boosted_variants_cos_kernel(const float* __restrict__ corpus, uint64_t n_rows, uint32_t dim, const float* __restrict__ queries,
                            uint32_t nv, uint32_t k, RowIds row_ids, const uint64_t* __restrict__ keys,
                            uint64_t* __restrict__ out_keys, float* __restrict__ out_cos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= k) return;  // wave-uniform
    const uint64_t key = keys[j];
    float c = 0.0f;
    if (key) {  // wave-uniform
        const uint64_t r = boosted_row_of(row_ids, n_rows, key_id(key));
        if constexpr (J > 0) {
            const int l32 = lane & 31;
            f32x4 x[J];
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + r * (128 * J)) + l32;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) x[jj] = p[jj * 32];
#pragma unroll 1
            for (uint32_t v = 0; v < nv; ++v) {
                f32x4 qf[1][J];
                const float qmag = load_query_fragment<J>(queries, v, l32, qf[0]);
                float dot[1];
                const float xmag = row_products<J, 1>(x, qf, dot);
                const float cv = cosine_of(half_allreduce_sum(dot[0]), qmag, xmag);
                c = (v == 0 || cv > c) ? cv : c;
            }
        } else {
            for (uint32_t v = 0; v < nv; ++v) {
                const float* qp = queries + (size_t)v * dim;
                const float cv = wave_row_cosine(corpus + r * dim, qp, dim, lane, wave_query_mag(qp, dim, lane));
                c = (v == 0 || cv > c) ? cv : c;
            }
        }
    }
    if (lane == 0) {
        out_cos[j] = c;
        if (out_keys) out_keys[j] = key;
    }
}

// ---- host side ------------------------------------------------------------------------------------------

namespace {

struct BoostedGroupedLaunch {
    const GroupedPlan& plan;
    const float* d_corpus;
    uint64_t n_rows;
    const uint32_t* d_list;
    const uint32_t* d_len;
    const float* d_queries;
    uint32_t nq, k;
    const uint32_t* d_dead;
    RowIds ids;
    const BoostView& bv;
    const GroupView& gv;
    uint64_t* d_partial;
    hipStream_t stream;
};

template <int J, int U, int QT, bool LIST>
void launch_bg_fast(const BoostedGroupedLaunch& a) {
    hipLaunchKernelGGL((scan_boosted_grouped_topk_kernel<J, U, QT, LIST>), dim3(a.plan.blocks, a.plan.passes), dim3(kBlock),
                       a.plan.lds_bytes, a.stream, a.d_corpus, a.n_rows, a.d_list, a.d_len, a.d_queries, a.nq, a.k, a.plan.kpad,
                       a.d_dead, a.ids, a.bv, a.gv, a.d_partial);
}

template <int J, int U, bool LIST>
void launch_bg_q(const BoostedGroupedLaunch& a) {
    switch (a.plan.qtile) {
        case 4: launch_bg_fast<J, U, 4, LIST>(a); break;
        case 2: launch_bg_fast<J, U, 2, LIST>(a); break;
        default: launch_bg_fast<J, U, 1, LIST>(a); break;
    }
}

template <bool LIST>
int32_t launch_bg(const BoostedGroupedLaunch& a, uint32_t dim) {
    const GroupedPlan& plan = a.plan;
    if (plan.deep && plan.qtile == 1 && grouped_fast_dim(dim)) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_bg_fast<3, 8, 1, LIST>(a);
        else if (dim == 768) launch_bg_fast<6, 4, 1, LIST>(a);
        else launch_bg_fast<8, 3, 1, LIST>(a);
    } else if (dim == 384) launch_bg_q<3, 4, LIST>(a);
    else if (dim == 768) launch_bg_q<6, 2, LIST>(a);
    else if (dim == 1024) launch_bg_q<8, 2, LIST>(a);
    else
        hipLaunchKernelGGL(scan_boosted_grouped_generic_kernel<LIST>, dim3(plan.blocks, a.nq), dim3(kBlock), plan.lds_bytes, a.stream,
                           a.d_corpus, a.n_rows, a.d_list, a.d_len, dim, a.d_queries, a.nq, a.k, plan.kpad, a.d_dead, a.ids, a.bv,
                           a.gv, a.d_partial);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace

int32_t launch_scan_boosted_grouped(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim,
                                    const uint32_t* d_list, const uint32_t* d_list_len, const float* d_queries, uint32_t nq,
                                    uint32_t k, const uint32_t* d_dead, RowIds ids, const BoostView& bv, const GroupView& gv,
                                    uint64_t* d_partial, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    if (bv.n_classes > CS_MAX_CLASSES || (bv.n_classes && !bv.weights) || !(bv.wmax >= 1.0f) || !(bv.wmin >= 0.0f && bv.wmin <= 1.0f))
        return fail(CS_ERR_BAD_ARG, "boosted scan needs its weight table, wmax >= 1 and 0 <= wmin <= 1");
    if (plan.lds_bytes > kGroupedLdsBudget || plan.kpad < k)
        return fail(CS_ERR_BAD_ARG, "grouped scan plan does not fit: %zu B of LDS, kpad %u for k %u", plan.lds_bytes, plan.kpad, k);
    if (d_list || d_list_len) {
        if (!d_list || !d_list_len) return fail(CS_ERR_BAD_ARG, "row list missing");
        return launch_bg<true>(BoostedGroupedLaunch{plan, d_corpus, 0, d_list, d_list_len, d_queries, nq, k, nullptr, ids, bv, gv,
                                                    d_partial, stream}, dim);
    }
    if (n_rows == 0) {  // nothing to score: all-empty lists
        CS_HIP(hipMemsetAsync(d_partial, 0, plan.partial_keys * sizeof(uint64_t), stream));
        return CS_OK;
    }
    return launch_bg<false>(BoostedGroupedLaunch{plan, d_corpus, n_rows, nullptr, nullptr, d_queries, nq, k, d_dead, ids, bv, gv,
                                                 d_partial, stream}, dim);
}

int32_t launch_boosted_variants_cos(const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nv,
                                    uint32_t k, RowIds ids, const uint64_t* d_keys, uint64_t* out_keys, float* out_cos,
                                    hipStream_t stream) {
    if (!d_keys || !out_cos || n_rows == 0 || nv == 0)
        return fail(CS_ERR_BAD_ARG, "boosted cosine pass needs keys, an output, a variant and a stored row");
    const dim3 grid((k + kWaves - 1) / kWaves);
    if (dim == 384) hipLaunchKernelGGL(boosted_variants_cos_kernel<3>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, nv, k, ids, d_keys, out_keys, out_cos);
    else if (dim == 768) hipLaunchKernelGGL(boosted_variants_cos_kernel<6>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, nv, k, ids, d_keys, out_keys, out_cos);
    else if (dim == 1024) hipLaunchKernelGGL(boosted_variants_cos_kernel<8>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, nv, k, ids, d_keys, out_keys, out_cos);
    else hipLaunchKernelGGL(boosted_variants_cos_kernel<0>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, nv, k, ids, d_keys, out_keys, out_cos);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
