// scan_similar_filter.hip — the refine and the fold of a similar-chunk search that runs through the filter (scan_filter.hip
// launch_scan_split with a SimilarRefine): the filter kernels, the phase plan, the prep kernel and the candidate buffers are
// the ordinary search's; only what becomes of a candidate differs.
//
//   refine   similar_rescore_kernel: rescore_keys_kernel (scan_filter.hip) restated — the same cosine, bit for bit — whose
//            final store writes the empty key for a row the query may not return: one not strictly above min_cos, the row
//            that carries the query's excluded id, a row of its excluded group (scan_similar.hip similar_keeps, restated).
//            similar_rescore_kernel<J, true> is its list form, as rescore_keys_kernel<J, true> is that kernel's: phase 0 of
//            a scoped call (a prepared plan, scoped_filter_plan.hpp) re-scores the scope's first c0 list entries.
//   fold     similar_select_kernel: select_candidates_kernel (scan_mfma.hip) restated, whose threshold never falls below
//            min_cos.
//
// The fold sees only the keys the refine leaves, so tau[q] is the k-th best cosine among the rows scanned so far that the
// query may return and that lie above the bound — or min_cos while there are fewer than k of them.  Either is a lower bound of
// the final k-th best of such rows, which is all the margin argument of scan_filter.hip's header asks of tau: every row
// whose exact cosine beats tau is a candidate, whatever the refine then makes of it.  The answer therefore equals the
// similar scan's (scan_similar.hip) bit for bit.  What the exclusions cost is candidates: the rows of an excluded file of
// near-duplicates all beat the k-th best of the others, and more than batched_cap(k) of them in one phase overflow the
// buffer — then index.hip answers from the similar scan.
// None of this asks where the row ranges or the bitmap come from: with a scope's prepared plan and its blocked-rows bitmap
// (index.hip run_similar_scoped) "the rows scanned so far" are the scope's, and the answer equals the scope's gathered
// similar scan (scan_similar.hip part 4) bit for bit; an overflow is then answered by that scan.
#include "scan.hpp"
#include "block_select.hpp"
#include "grouped_plan.hpp"  // kNoGroup

namespace cs {

typedef float sf_f32x4 __attribute__((ext_vector_type(4)));

// scan_filter.hip's and scan_mfma.hip's launch constants, restated (scan.hpp kSelThreads / kSelCap are asserted there)
constexpr int SRK_THREADS = 256;
constexpr int SSEL_THREADS = (int)kSelThreads;
constexpr int SSEL_CAP = (int)kSelCap;

__device__ __forceinline__ float sf_half_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// scan_similar.hip's, restated: the group of an id under the table as the kernels read it
__device__ __forceinline__ uint32_t sf_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;  // ids past the table (appended after the last assignment) are ungrouped
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

// Refine: rescore_keys_kernel<J, false> with the similar search's final store.  Grid dim3(rk_blocks, nq); candidate i of
// query q is the row in the low word of cand[q][i], or row i in phase 0 (first_rows != 0), where tombstoned rows become
// empty keys.  The key is 0 unless the cosine is finite and > min_cos (-inf: no bound) and the row is kept; the bound is
// tested first, then the id, then — only for a query that excludes a group — the row's group: one 4-byte table read per
// candidate that survived the first two.  ex_ids[q] and ex_groups[q] are block-uniform (q = blockIdx.y).
// LIST (phase 0 of a scoped call, scoped_filter_plan.hpp; first_rows != 0): candidate i is row dead[i] — the scope's ascending
// row list is passed where the bitmap goes, as to rescore_keys_kernel<J, true>; it holds live, allowed rows only, so no bit
// is tested.  The exclusions are: a source inside the scope, and the rows of its file, are list entries like any other.
template <int J, bool LIST = false>
__global__ void __launch_bounds__(SRK_THREADS)
similar_rescore_kernel(const float* __restrict__ corpus, const float* __restrict__ queries, const float* __restrict__ qmag,
                       uint64_t* __restrict__ cand, const uint32_t* __restrict__ cnt, uint32_t cap, RowIds id_base,
                       uint32_t first_rows, const uint32_t* __restrict__ dead, GroupView gv,
                       const uint32_t* __restrict__ ex_ids, const uint32_t* __restrict__ ex_groups, float min_cos) {
    constexpr int DIM = 128 * J;
    constexpr int RU = J <= 3 ? 4 : 2;            // rows per half-wave per round, loads issued together
    constexpr int PER = RU * (SRK_THREADS / 32);  // candidates per block per round
    const int tid = threadIdx.x, l32 = tid & 31;
    const uint32_t hw = tid >> 5;
    const uint32_t q = blockIdx.y;
    uint32_t n = first_rows ? first_rows : cnt[(size_t)q * kCntStride];
    if (n > cap) n = cap;  // similar_select_kernel raises the overflow flag
    if (blockIdx.x * PER >= n) return;
    sf_f32x4 qf[J];
    {
        const sf_f32x4* qp = reinterpret_cast<const sf_f32x4*>(queries + (size_t)q * DIM) + l32;
#pragma unroll
        for (int j = 0; j < J; ++j) qf[j] = qp[j * 32];
    }
    const float qm = qmag[q];
    const uint32_t ex_id = ex_ids[q], ex_group = ex_groups[q];
    uint64_t* slots = cand + (size_t)q * cap;
    for (uint32_t i0 = blockIdx.x * PER; i0 < n; i0 += gridDim.x * PER) {
        sf_f32x4 v[RU][J];
        uint32_t row[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (SRK_THREADS / 32) + hw;  // half-wave uniform
            row[u] = (i < n) ? (first_rows ? (LIST ? dead[i] : i) : (uint32_t)slots[i]) : 0u;
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (SRK_THREADS / 32) + hw;
            if (i < n) {
                const sf_f32x4* p = reinterpret_cast<const sf_f32x4*>(corpus + (size_t)row[u] * DIM) + l32;
#pragma unroll
                for (int j = 0; j < J; ++j) v[u][j] = p[j * 32];
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (SRK_THREADS / 32) + hw;
            if (i < n) {  // xor masks <= 16 stay inside the half-wave
                float ss = 0.0f, dot = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    ss = fmaf(v[u][j].x, v[u][j].x, ss); ss = fmaf(v[u][j].y, v[u][j].y, ss);
                    ss = fmaf(v[u][j].z, v[u][j].z, ss); ss = fmaf(v[u][j].w, v[u][j].w, ss);
                    dot = fmaf(v[u][j].x, qf[j].x, dot); dot = fmaf(v[u][j].y, qf[j].y, dot);
                    dot = fmaf(v[u][j].z, qf[j].z, dot); dot = fmaf(v[u][j].w, qf[j].w, dot);
                }
                const float xmag = sqrtf(sf_half_sum(ss));
                const float d = sf_half_sum(dot);
                const float c = (qm == 0.0f || xmag == 0.0f) ? 0.0f : d / (qm * xmag);  // batch.rs:320-323
                // NaN/Inf scores are never returned
                const bool live = LIST || !(first_rows && dead) || !((dead[row[u] >> 5] >> (row[u] & 31)) & 1u);
                if (l32 == 0) {
                    uint64_t key = 0ull;
                    if (live && c > -__builtin_huge_valf() && c < __builtin_huge_valf() && c > min_cos) {
                        const uint32_t id = id_base.of(row[u]);
                        if (id != ex_id && (ex_group == kNoGroup || sf_group_of(gv, id) != ex_group)) key = key_pack(c, id);
                    }
                    slots[i] = key;
                }
            }
        }
    }
}

// Fold: select_candidates_kernel with a floor under the threshold.  One block per query.
//   carry[q][k]   : best k keys so far (0 = empty), best first; updated in place
//   tau[q]        : cosine of the k-th best if k keys have been kept, else min_cos
//   cnt[q]        : reset to 0;  overflow[0] |= 1 if cnt[q] > cap
// Every key in the list is above min_cos already (the refine), so the floor only replaces the -inf of a list that is not
// full.  Without it a call whose bound leaves fewer than k rows would keep tau = -inf to the end: every row of every later
// phase would be a candidate and the buffer would overflow — for a search whose answer is a handful of rows, or none.
__global__ void __launch_bounds__(SSEL_THREADS)
similar_select_kernel(const uint64_t* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap, uint32_t k,
                      uint64_t* __restrict__ carry, float* __restrict__ tau, uint32_t* __restrict__ overflow, int final_out,
                      float min_cos, uint64_t* __restrict__ out_keys, float* __restrict__ out_cos,
                      uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_counts) {
    __shared__ __attribute__((aligned(16))) uint64_t a[SSEL_CAP];
    __shared__ uint32_t live;
    __shared__ uint32_t sel_slots[66];
    const int tid = threadIdx.x;
    const uint32_t q = blockIdx.x;
    uint32_t n = cnt[(size_t)q * kCntStride];
    if (n > cap) {
        if (tid == 0) { atomicOr(overflow, 1u); if (gridDim.x > kGatedMaxQ) atomicOr(overflow + 1, 1u); }
        n = cap;
    }
    const uint64_t* src = cand + (size_t)q * cap;
    for (uint32_t i = tid; i < SSEL_CAP; i += SSEL_THREADS) a[i] = (i < k) ? carry[(size_t)q * k + i] : 0ull;
    if (tid == 0) live = 0;
    __syncthreads();
    const uint32_t room = SSEL_CAP - k;
    for (uint32_t done = 0; done < n || done == 0; done += room) {
        const uint32_t take = (n - done) < room ? (n - done) : room;
        // sort size: the k carried keys + this chunk, padded with zero keys to a power of two
        uint32_t nsort = 64;
        while (nsort < k + take) nsort <<= 1;
        for (uint32_t i = tid; k + i < nsort; i += SSEL_THREADS) a[k + i] = (i < take) ? src[done + i] : 0ull;
        if (nsort > 256) {  // hundreds of candidates: bracket the k-th key first, sort only what is above it
            __syncthreads();
            nsort = block_select_topk<SSEL_THREADS, SSEL_CAP / SSEL_THREADS>(a, k + take, k, tid, sel_slots);
        }
        uint32_t prev_stride = 128;  // block barrier only around cross-segment stages (block_bitonic_desc, scan.hip)
        for (uint32_t size = 2; size <= nsort; size <<= 1)
            for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
                if (stride >= 128 || prev_stride >= 128) {
                    __syncthreads();
                } else {
                    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
                prev_stride = stride;
                for (uint32_t t = tid; t < nsort / 2; t += SSEL_THREADS) {
                    const uint32_t i = 2 * t - (t & (stride - 1)), j = i + stride;
                    const uint64_t x = a[i], y = a[j];
                    if ((x < y) == ((i & size) == 0)) { a[i] = y; a[j] = x; }
                }
            }
        __syncthreads();
        if (n == 0) break;
    }
    for (uint32_t i = tid; i < k; i += SSEL_THREADS) {
        const uint64_t key = a[i];
        carry[(size_t)q * k + i] = key;
        if (final_out) {
            if (key) atomicAdd(&live, 1u);
            if (out_keys) out_keys[(size_t)q * k + i] = key;
            if (out_cos) out_cos[(size_t)q * k + i] = key ? key_cos(key) : 0.0f;
            if (out_ids) out_ids[(size_t)q * k + i] = key ? key_id(key) : 0xffffffffu;
        }
    }
    if (tid == 0) {
        const uint64_t kth = a[k - 1];
        tau[q] = kth ? key_cos(kth) : min_cos;
        cnt[(size_t)q * kCntStride] = 0;
    }
    __syncthreads();
    if (final_out && out_counts && tid == 0) out_counts[q] = live;
}

static int32_t check_similar_view(const SimilarView& sv) {
    if (!sv.d_ex_ids || !sv.d_ex_groups || sv.min_cos != sv.min_cos)
        return fail(CS_ERR_BAD_ARG, "similar refine needs its exclusion arrays and a bound that is a number");
    return CS_OK;
}

template <int J>
static void similar_rescore_launch(const dim3 grid, hipStream_t stream, const float* d_corpus, const float* d_queries,
                                   const float* d_qmag, const BatchedState& st, uint32_t cap, RowIds ids, uint32_t first_rows,
                                   const uint32_t* d_dead, const uint32_t* d_list, const GroupView& gv, const SimilarView& sv) {
    if (first_rows && d_list)
        hipLaunchKernelGGL((similar_rescore_kernel<J, true>), grid, dim3(SRK_THREADS), 0, stream, d_corpus, d_queries, d_qmag,
                           st.d_cand, st.d_cnt, cap, ids, first_rows, d_list, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos);
    else
        hipLaunchKernelGGL(similar_rescore_kernel<J>, grid, dim3(SRK_THREADS), 0, stream, d_corpus, d_queries, d_qmag, st.d_cand,
                           st.d_cnt, cap, ids, first_rows, d_dead, gv, sv.d_ex_ids, sv.d_ex_groups, sv.min_cos);
}

int32_t launch_similar_rescore(const BatchedState& st, const SplitQueryWs& qw, const float* d_corpus, uint32_t dim,
                               const float* d_queries, uint32_t nq, uint32_t cap, uint32_t rk_blocks, uint32_t first_rows,
                               const uint32_t* d_dead, RowIds ids, const GroupView& gv, const SimilarView& sv,
                               hipStream_t stream, const uint32_t* d_list) {
    CS_TRY(check_similar_view(sv));
    if (rk_blocks == 0 || nq == 0) return fail(CS_ERR_BAD_ARG, "similar refine: empty grid");
    if (d_list && first_rows > cap) return fail(CS_ERR_BAD_ARG, "similar refine: a phase-0 list of %u rows does not fit", first_rows);
    const dim3 grid(rk_blocks, nq);
    if (dim == 384)
        similar_rescore_launch<3>(grid, stream, d_corpus, d_queries, qw.d_qmag, st, cap, ids, first_rows, d_dead, d_list, gv, sv);
    else if (dim == 768)
        similar_rescore_launch<6>(grid, stream, d_corpus, d_queries, qw.d_qmag, st, cap, ids, first_rows, d_dead, d_list, gv, sv);
    else if (dim == 1024)
        similar_rescore_launch<8>(grid, stream, d_corpus, d_queries, qw.d_qmag, st, cap, ids, first_rows, d_dead, d_list, gv, sv);
    else
        return fail(CS_ERR_UNSUPPORTED, "similar refine supports dim 384/768/1024, got %u", dim);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_similar_select(const BatchedState& st, uint32_t nq, uint32_t cap, uint32_t k, bool last, const SimilarView& sv,
                              uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_counts,
                              hipStream_t stream) {
    if (sv.min_cos != sv.min_cos) return fail(CS_ERR_BAD_ARG, "similar fold needs a bound that is a number");
    if (k == 0 || k > (uint32_t)SSEL_CAP / 4) return fail(CS_ERR_BAD_ARG, "similar fold: k %u does not fit", k);
    hipLaunchKernelGGL(similar_select_kernel, dim3(nq), dim3(SSEL_THREADS), 0, stream, st.d_cand, st.d_cnt, cap, k, st.d_carry,
                       st.d_tau, st.d_overflow, last ? 1 : 0, sv.min_cos, d_out_keys, d_out_cos, d_out_ids, d_out_counts);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
