// scan_boosted.hip — the boosted search: the exact best k live rows under per-class score weights.  The reference
// re-weights hits by what they are — a structural query multiplies the score of every hit of that ChunkKind by 1.15
// (src/search/mod.rs:238-252), a primary language multiplies its hits by 1.20 (:789-806) — but only the retrieval_limit hits
// it has already ranked, and re-sorts them: a chunk of the wanted kind just outside the fetched list never rises into it.
// Here the weight is part of the selection (the contract: include/codesearch_gpu.h).
//
//   c = the streaming scan's cosine of the row (scan_wave.hpp's functions, so its bits by construction)
//   s = 1.0f - (1.0f - c) * 0.5f     the reference's score (store.rs:478); the multiply is exact, so a fused form is the same
//   b = s * w                        w = weights[class of the row's id], 1 for an id without a class or a class past the table
//   the answer = the k live rows with the largest key_pack(b, id)
//
//   1. boosted scan: scan_topk_kernel's tile loop (scan.hip) over every stored row, or over a scope's row list as the
//      gathered scan reads it (scan_masked.hip) — one body, LIST chooses the addressing.  The value inserted is b and the
//      gate `b > thr` stays the whole test: ids still arrive ascending, so a row that ties the worst b loses to it.  No class
//      is read for most rows: with wmax = the largest weight a row can take (the table's maximum, or 1 if that is larger),
//      fl(s * wmax) <= thr rejects a row on the fast path — rounding is monotone, so w <= wmax gives fl(s * w) <=
//      fl(s * wmax) for s >= 0.  (s < 0 needs c < -1, a rounding excess of a row opposite to the query; the bound of its b
//      is then s * wmin, wmin = the smallest weight a row can take: boosted_bound selects.)  Only the rows past that
//      pre-gate take the slow path, read classes[id - id_base] and the weight, and are tested again with their own b.
//      The weight table (<= 16 KB) stays in global memory, read through L2: plan_scan already fills the 64 KB a block may
//      ask for without an attribute (two queries at kpad 1024), and only slow-path rows read it, one address per wave.
//      Prime pass (PRIME, scan.hip "Primed scans"): the same pass over a prefix keeps one number per wave and query, the
//      best b of a live row it met — so it reads the class of every row that raises its maximum — and the k-th largest of
//      those maxima, attained by k different rows, bounds the k-th best b from below.  The full scan starts its lists from
//      the float just below it.  Beside sparing a long list its fill phase this is what makes the pre-gate tight: a
//      wave's own k-th best b is far below the store's when the heaviest class is rare.  No gate word.
//   2. merge: the lists hold packed keys of b; block_merge_store and launch_merge order keys of any float.
//   3. cosine of the winners: the merged keys carry b and the id, not c.  boosted_cos_kernel takes the nq x k winners,
//      finds each id's stored row (rows are stored in ascending id: the identity, or a bisection over the row -> id table)
//      and scores it again with the same functions: the same bits.  It also hands the keys on to the host's pinned buffer,
//      so the host-buffer call makes no extra round trip.
#include "scan.hpp"
#include "scan_wave.hpp"
#include "scan_rules.hpp"

namespace cs {

static_assert(CS_MAX_CLASSES <= CS_NO_CLASS, "a class past every table must exist");

// boosted_score (s of c), boosted_bound (the pre-gate's value), boosted_weight (w of an id) and boosted_row_of (the stored
// row of a winner's id): scan_rules.hpp.

// ---- 1. boosted scan --------------------------------------------------------------------------------------
// scan_topk_kernel (scan.hip) without the gate word: see there for J, U, QT and PRIME.  LIST: half-wave h of tile t
// takes row rows[t * 2U + 2u + h] of rows[0, *rows_len) (live rows only, ascending: no tombstone read) — a prime pass
// the first min(n_rows, *rows_len) of them; else row t * 2U + 2u + h of [0, n_rows).
//
// Registers: plan_scan sizes the grid to be fully resident from the streaming scan's occupancy; at 384-d with four queries
// per pass that is three blocks per CU, 168 VGPRs.  Like scan_similar_list_kernel that shape declares the three waves per
// SIMD it is launched for; every other shape is launched at one or two blocks per CU.
template <int J, int QT>
constexpr int boosted_waves_per_simd() { return (J == 3 && QT == 4) ? 3 : 1; }

template <int J, int U, int QT, bool LIST, bool PRIME>
__global__ void __launch_bounds__(kBlock, (boosted_waves_per_simd<J, QT>()))
scan_boosted_topk_kernel(const float* __restrict__ corpus, uint64_t n_rows, const uint32_t* __restrict__ rows,
                         const uint32_t* __restrict__ rows_len, const float* __restrict__ queries, uint32_t nq, uint32_t k,
                         uint32_t kpad, const uint32_t* __restrict__ dead, RowIds row_ids, BoostView bv,
                         uint64_t* __restrict__ partial, const float* __restrict__ floor_in, float* __restrict__ wave_max,
                         uint32_t* __restrict__ done_ctr, float* __restrict__ floor_out) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad]
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;
    uint64_t n = n_rows;
    if constexpr (LIST) {
        const uint64_t len = *rows_len;
        n = (PRIME && n_rows < len) ? n_rows : len;
    }

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
    float thr[QT], floor[QT];
    uint32_t wpos[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        const uint32_t q = (q0 + qi < nq) ? (q0 + qi) : (nq - 1);
        qmag[qi] = load_query_fragment<J>(queries, q, l32, qf[qi]);
        floor[qi] = (!PRIME && floor_in) ? floor_in[q] : -__builtin_huge_valf();
        thr[qi] = floor[qi];  // PRIME: the lane's running maximum of b
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
            for (int j = 0; j < J; ++j) {
                if constexpr (PRIME) x[u][j] = p[j * 32];  // cached: the full scan re-reads these rows right after
                else x[u][j] = __builtin_nontemporal_load(p + j * 32);
            }
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
                if constexpr (PRIME) {  // the half-wave's own row: a class is read only for a row that may raise the maximum
                    if (valid && boosted_bound(s, wmin, wmax) > thr[qi]) {
                        const uint64_t rr = LIST ? (uint64_t)row[u] : e0 + 2 * u + half;
                        if (LIST || !row_is_dead(dead, rr)) {
                            const float b = s * boosted_weight(bv, row_ids.of(rr));
                            if (b > thr[qi]) thr[qi] = b;
                        }
                    }
                    continue;
                }
                unsigned long long m = __ballot(valid && l32 == 0 && boosted_bound(s, wmin, wmax) > thr[qi]);  // the pre-gate: no class read
                if (m) {  // wave-uniform slow path; half 0 (the lower row, the lower id) first
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float ss = __shfl(s, src, 64);
                        const uint64_t rr = LIST ? (uint64_t)__shfl(row[u], src, 64) : e0 + 2 * u + (src >> 5);
                        if (boosted_bound(ss, wmin, wmax) > thr[qi] && (LIST || !row_is_dead(dead, rr))) {
                            const uint32_t id = row_ids.of(rr);
                            const float b = ss * boosted_weight(bv, id);
                            if (b > thr[qi]) wave_list_insert(list, k, lane, b, id, thr[qi], wpos[qi], floor[qi]);
                        }
                    }
                }
            }
        }
    }
    if constexpr (PRIME) {
        prime_pass_tail<QT>(thr, q0, nq, k, gw, tid, lane, lds_keys, wave_max, done_ctr, floor_out);
        return;
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

// Any other dim: one wave per row (LIST: per list entry), lanes stride over columns (wave_row_cosine, scan_wave.hpp).
template <bool LIST>
__global__ void __launch_bounds__(kBlock)
scan_boosted_generic_kernel(const float* __restrict__ corpus, uint64_t n_rows, const uint32_t* __restrict__ rows,
                            const uint32_t* __restrict__ rows_len, uint32_t dim, const float* __restrict__ queries, uint32_t nq,
                            uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds row_ids, BoostView bv,
                            uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    const uint64_t n = LIST ? (uint64_t)*rows_len : n_rows;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    const float wmin = bv.wmin, wmax = bv.wmax;
    float thr = -__builtin_huge_valf();
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t e = gw; e < n; e += nw) {
        const uint64_t r = LIST ? (uint64_t)rows[e] : e;
        const float s = boosted_score(wave_row_cosine(corpus + r * dim, qp, dim, lane, qmag));
        if (boosted_bound(s, wmin, wmax) > thr && (LIST || !row_is_dead(dead, r))) {  // wave-uniform
            const uint32_t id = row_ids.of(r);
            const float b = s * boosted_weight(bv, id);
            if (b > thr) wave_list_insert(list, k, lane, b, id, thr, wpos);
        }
    }
    __syncthreads();
    block_merge_store(lds_keys, kpad, k, q, tid, partial);
}

// ---- 3. cosine of the winners ---------------------------------------------------------------------------------
// Wave (blockIdx.x * kWaves + wave) of query blockIdx.y takes winner j of keys[q][k]: out_cos[q][j] = the streaming
// scan's cosine of the row (0 for an empty slot), out_keys[q][j] = the key (optional).  J = dim / 128 for the tuned dims
// — both half-waves score the row, as either would in the scan — and 0 for any other dim.
template <int J>
__global__ void __launch_bounds__(kBlock)
boosted_cos_kernel(const float* __restrict__ corpus, uint64_t n_rows, uint32_t dim, const float* __restrict__ queries, uint32_t k,
                   RowIds row_ids, const uint64_t* __restrict__ keys, uint64_t* __restrict__ out_keys,
                   float* __restrict__ out_cos) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.y;
    const uint32_t j = blockIdx.x * kWaves + wave;
    if (j >= k) return;  // wave-uniform
    const size_t slot = (size_t)q * k + j;
    const uint64_t key = keys[slot];
    float c = 0.0f;
    if (key) {  // wave-uniform
        const uint64_t r = boosted_row_of(row_ids, n_rows, key_id(key));
        if constexpr (J > 0) {
            const int l32 = lane & 31;
            f32x4 qf[1][J], x[J];
            const float qmag = load_query_fragment<J>(queries, q, l32, qf[0]);
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + r * (128 * J)) + l32;
#pragma unroll
            for (int jj = 0; jj < J; ++jj) x[jj] = p[jj * 32];
            float dot[1];
            const float xmag = row_products<J, 1>(x, qf, dot);
            c = cosine_of(half_allreduce_sum(dot[0]), qmag, xmag);
        } else {
            const float* qp = queries + (size_t)q * dim;
            c = wave_row_cosine(corpus + r * dim, qp, dim, lane, wave_query_mag(qp, dim, lane));
        }
    }
    if (lane == 0) {
        out_cos[slot] = c;
        if (out_keys) out_keys[slot] = key;
    }
}

// ---- host side ------------------------------------------------------------------------------------------

namespace {

// One boosted scan launch: every stored row [0, n_rows), or the list d_list[0, *d_len); prime + prime_pass: the prime
// pass over the first n_rows rows / list entries instead (plan from plan_prime); prime alone: the lists start from
// prime->d_floor.
struct BoostedLaunch {
    const ScanPlan& plan;
    const float* d_corpus;
    uint64_t n_rows;
    const uint32_t* d_list;
    const uint32_t* d_len;
    const float* d_queries;
    uint32_t nq, k;
    const uint32_t* d_dead;
    RowIds ids;
    const BoostView& bv;
    uint64_t* d_partial;
    const ScanPrime* prime;
    bool prime_pass;
    hipStream_t stream;
};

template <int J, int U, int QT, bool LIST>
void launch_boosted_fast(const BoostedLaunch& a) {
    const size_t lds = (size_t)QT * kWaves * a.plan.kpad * sizeof(uint64_t);
    const dim3 grid(a.plan.blocks, a.plan.passes);
    if (a.prime_pass)
        hipLaunchKernelGGL((scan_boosted_topk_kernel<J, U, QT, LIST, true>), grid, dim3(kBlock), lds, a.stream, a.d_corpus, a.n_rows,
                           a.d_list, a.d_len, a.d_queries, a.nq, a.k, a.plan.kpad, a.d_dead, a.ids, a.bv, nullptr, nullptr,
                           a.prime->d_wave_max, a.prime->d_done, a.prime->d_floor);
    else
        hipLaunchKernelGGL((scan_boosted_topk_kernel<J, U, QT, LIST, false>), grid, dim3(kBlock), lds, a.stream, a.d_corpus, a.n_rows,
                           a.d_list, a.d_len, a.d_queries, a.nq, a.k, a.plan.kpad, a.d_dead, a.ids, a.bv, a.d_partial,
                           a.prime ? a.prime->d_floor : nullptr, nullptr, nullptr, nullptr);
}

template <int J, int U, bool LIST>
void launch_boosted_q(const BoostedLaunch& a) {
    switch (a.plan.qtile) {
        case 4: launch_boosted_fast<J, U, 4, LIST>(a); break;
        case 2: launch_boosted_fast<J, U, 2, LIST>(a); break;
        default: launch_boosted_fast<J, U, 1, LIST>(a); break;
    }
}

template <bool LIST>
int32_t launch_boosted(const BoostedLaunch& a, uint32_t dim) {
    const BoostView& bv = a.bv;
    if (bv.n_classes > CS_MAX_CLASSES || (bv.n_classes && !bv.weights) || !(bv.wmax >= 1.0f) || !(bv.wmin >= 0.0f && bv.wmin <= 1.0f))
        return fail(CS_ERR_BAD_ARG, "boosted scan needs its weight table, wmax >= 1 and 0 <= wmin <= 1");
    const ScanPlan& plan = a.plan;
    if (plan.kpad < a.k || plan.qtile < 1 || (size_t)plan.qtile * kWaves * plan.kpad * sizeof(uint64_t) > 64 * 1024)
        return fail(CS_ERR_BAD_ARG, "boosted scan plan does not fit: qtile %u, kpad %u for k %u", plan.qtile, plan.kpad, a.k);
    const bool fast = dim == 384 || dim == 768 || dim == 1024;
    if (a.prime_pass && (!fast || !a.prime || a.n_rows == 0 || plan.blocks * (uint32_t)kWaves > kWaves * plan.kpad))
        return fail(CS_ERR_BAD_ARG, "boosted prime pass needs a tuned dim, its buffers, rows and at most kpad blocks");
    if (fast && plan.deep && plan.qtile == 1) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_boosted_fast<3, 8, 1, LIST>(a);
        else if (dim == 768) launch_boosted_fast<6, 4, 1, LIST>(a);
        else launch_boosted_fast<8, 3, 1, LIST>(a);
    } else if (dim == 384) launch_boosted_q<3, 4, LIST>(a);
    else if (dim == 768) launch_boosted_q<6, 2, LIST>(a);
    else if (dim == 1024) launch_boosted_q<8, 2, LIST>(a);
    else {
        const size_t lds = (size_t)kWaves * plan.kpad * sizeof(uint64_t);
        hipLaunchKernelGGL(scan_boosted_generic_kernel<LIST>, dim3(plan.blocks, a.nq), dim3(kBlock), lds, a.stream, a.d_corpus,
                           a.n_rows, a.d_list, a.d_len, dim, a.d_queries, a.nq, a.k, plan.kpad, a.d_dead, a.ids, bv, a.d_partial);
    }
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace

int32_t launch_scan_boosted(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries,
                            uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const BoostView& bv,
                            uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime, bool prime_pass) {
    if (n_rows == 0 && !prime_pass) {  // nothing to score: all-empty partial lists
        CS_HIP(hipMemsetAsync(d_partial, 0, plan.partial_keys * sizeof(uint64_t), stream));
        return CS_OK;
    }
    return launch_boosted<false>(BoostedLaunch{plan, d_corpus, n_rows, nullptr, nullptr, d_queries, nq, k, d_dead, ids, bv,
                                               d_partial, prime, prime_pass, stream}, dim);
}

int32_t launch_scan_boosted_list(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const BoostView& bv, uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime,
                                 bool prime_pass, uint64_t prime_rows) {
    if (!d_list || !d_list_len) return fail(CS_ERR_BAD_ARG, "boosted scan over a row list needs the list and its length");
    return launch_boosted<true>(BoostedLaunch{plan, d_corpus, prime_pass ? prime_rows : 0, d_list, d_list_len, d_queries, nq, k,
                                              nullptr, ids, bv, d_partial, prime, prime_pass, stream}, dim);
}

int32_t launch_boosted_cos(const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nq, uint32_t k,
                           RowIds ids, const uint64_t* d_keys, uint64_t* out_keys, float* out_cos, hipStream_t stream) {
    if (!d_keys || !out_cos || n_rows == 0) return fail(CS_ERR_BAD_ARG, "boosted cosine pass needs keys, an output and a stored row");
    const dim3 grid((k + kWaves - 1) / kWaves, nq);
    if (dim == 384) hipLaunchKernelGGL(boosted_cos_kernel<3>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, k, ids, d_keys, out_keys, out_cos);
    else if (dim == 768) hipLaunchKernelGGL(boosted_cos_kernel<6>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, k, ids, d_keys, out_keys, out_cos);
    else if (dim == 1024) hipLaunchKernelGGL(boosted_cos_kernel<8>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, k, ids, d_keys, out_keys, out_cos);
    else hipLaunchKernelGGL(boosted_cos_kernel<0>, grid, dim3(kBlock), 0, stream, d_corpus, n_rows, dim, d_queries, k, ids, d_keys, out_keys, out_cos);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
