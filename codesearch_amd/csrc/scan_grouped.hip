// scan_grouped.hip — the grouped search: the exact best k live rows such that no group (a chunk's file) contributes more
// than per_group of them.  The reference caps hits per file only after ranking (src/search/mod.rs:1007-1038 `--per-file`,
// :947-957 `--compact`): a file with many near-duplicate chunks fills the ranked list before the cap is applied.
// Host plan, the contract and the merge lemma: grouped_plan.hpp.
//
//   1. capped scan: scan_topk_kernel's tile loop (scan.hip), a row scored by the functions that score it there
//      (scan_wave.hpp: load_query_fragment, row_products, cosine_of — so every cosine is bit-identical), with a u32
//      group slot beside every key slot of a wave's list.  The fast-path gate stays `c > thr`: a full list whose worst
//      key the row does not beat holds k cap-valid rows that all beat it.  On the slow path the row's group comes from
//      the table (one address per wave) and the insert keeps the list the capped top-k of what the wave has met:
//      wave_list_insert_grouped.  No prime pass, and no block merge: each wave's list goes to HBM as it is.
//   2. capped merge: every level sorts its keys, ranks each key inside its group and drops ranks >= per_group BEFORE it
//      keeps the best k: merge_topk_grouped_kernel.
//   1b. gathered capped scan: step 1 over a scope's row list, read as the masked scan reads it (scan_masked.hip):
//      scan_grouped_list_topk_kernel.  The same per-wave lists, the same merge.
//   3. capped variants merge: the capped lists of up to nine query variants -> one capped list in which a chunk keeps its
//      best key; every level de-duplicates and caps: merge_variants_grouped_kernel.
#include "scan.hpp"
#include "grouped_plan.hpp"
#include "scan_wave.hpp"
#include "scan_rules.hpp"

namespace cs {

static_assert(kNoGroup == CS_NO_GROUP, "grouped_plan.hpp restates the public constant");

// group_of, wave_list_insert_grouped (the capped insert of a wave's list) and wave_list_store: scan_rules.hpp.

// ---- 1. capped scan ---------------------------------------------------------------------------------
// scan_topk_kernel (scan.hip) without PRIME, the floor and the gate: see there for J, U and QT.
template <int J, int U, int QT>
__global__ void __launch_bounds__(kBlock)
scan_grouped_topk_kernel(const float* __restrict__ corpus, uint64_t n_rows, const float* __restrict__ queries, uint32_t nq,
                         uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds id_base, GroupView gv,
                         uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)QT * kWaves * kpad);
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi)
        qmag[qi] = load_query_fragment<J>(queries, (q0 + qi < nq) ? (q0 + qi) : (nq - 1), l32, qf[qi]);
    float thr[QT];
    uint32_t wpos[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        thr[qi] = -__builtin_huge_valf();
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
                if (m) {  // wave-uniform slow path; every row takes it until the list is full
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    volatile uint32_t* glist = lds_groups + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float cc = __shfl(c, src, 64);
                        const uint64_t rr = row0 + 2 * u + (src >> 5);
                        if (cc > thr[qi] && !row_is_dead(dead, rr)) {
                            const uint32_t id = id_base.of(rr);
                            wave_list_insert_grouped(list, glist, k, gv.per_group, lane, cc, id, group_of(gv, id), thr[qi],
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

// Any other dim: one wave per row, lanes stride over columns.
__global__ void __launch_bounds__(kBlock)
scan_grouped_generic_kernel(const float* __restrict__ corpus, uint64_t n_rows, uint32_t dim, const float* __restrict__ queries,
                            uint32_t nq, uint32_t k, uint32_t kpad, const uint32_t* __restrict__ dead, RowIds id_base,
                            GroupView gv, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)kWaves * kpad);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }
    const float* qp = queries + (size_t)q * dim;
    // (this kernel keeps its own text of wave_query_mag / wave_row_cosine, scan_wave.hpp: with either helper, or cosine_of,
    // it compiles 2 instructions longer; the arithmetic is the same, line for line)
    float s = 0.0f;
    for (uint32_t c = lane; c < dim; c += 64) s = fmaf(qp[c], qp[c], s);
    const float qmag = sqrtf(wave_allreduce_sum(s));
    float thr = -__builtin_huge_valf();
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    volatile uint32_t* glist = lds_groups + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t r = gw; r < n_rows; r += nw) {
        const float* xp = corpus + r * dim;
        float ss = 0.0f, dot = 0.0f;
        for (uint32_t c = lane; c < dim; c += 64) {
            const float v = xp[c];
            ss = fmaf(v, v, ss);
            dot = fmaf(v, qp[c], dot);
        }
        const float xmag = sqrtf(wave_allreduce_sum(ss));
        const float d = wave_allreduce_sum(dot);
        const float c = (qmag == 0.0f || xmag == 0.0f) ? 0.0f : d / (qmag * xmag);
        if (c > thr && !row_is_dead(dead, r)) {  // wave-uniform
            const uint32_t id = id_base.of(r);
            wave_list_insert_grouped(list, glist, k, gv.per_group, lane, c, id, group_of(gv, id), thr, wpos);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    wave_list_store(lds_keys + (size_t)wave * kpad, k, lane, partial, q, wave);
}

// ---- 2. capped merge ---------------------------------------------------------------------------------
// merge_topk_kernel's list layout (scan.hip): list l of query q starts at in + q * q_stride + l * k; block (g, q) takes
// lists [g * G, min(nlists, (g + 1) * G)) and writes its capped best k to out_keys[q][g][k], best first; with one block
// per query the result is final and is also decoded to cos / ids / counts.  Per block:
//   a[] = the keys, sorted: position = rank under (cosine desc, id asc);
//   b[] = (group << 32 | ~position) images of the non-empty keys, sorted: a group's keys are neighbours, best first, so
//         a key is past the cap exactly when the image per_group places before it has the same group;
//   those keys are zeroed in a[], and the survivors — still in key order — are compacted; the first k leave.
// block_select_topk is not used: it would discard, before the cap, rows that the cap promotes.
constexpr int kGMergeBlock = 1024;
constexpr int kGMergePer = kGroupedMergeCap / kGMergeBlock;

__global__ void __launch_bounds__(kGMergeBlock)
merge_topk_grouped_kernel(const uint64_t* __restrict__ in, uint32_t nlists, uint32_t k, uint32_t G, uint64_t q_stride,
                          GroupView gv, uint64_t* __restrict__ out_keys, float* __restrict__ out_cos,
                          uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) uint64_t a[];  // [nsort] keys, [nsort] images
    __shared__ uint32_t wave_tot[kGMergeBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x, q = blockIdx.y, ngroups = gridDim.x;
    const uint32_t lo = g * G;
    const uint32_t hi = (lo + G < nlists) ? lo + G : nlists;
    const uint32_t ncand = (hi - lo) * k;  // <= kGroupedMergeCap (the launcher's G)
    uint32_t nsort = 64;
    while (nsort < ncand) nsort <<= 1;
    uint64_t* const b = a + nsort;
    const uint64_t* src = in + (size_t)q * q_stride + (size_t)lo * k;
    for (uint32_t i = tid; i < nsort; i += kGMergeBlock) a[i] = (i < ncand) ? src[i] : 0ull;
    block_bitonic_desc<kGMergeBlock>(a, nsort, tid);
    for (uint32_t i = tid; i < nsort; i += kGMergeBlock) {
        const uint64_t key = a[i];
        b[i] = key ? (((uint64_t)group_of(gv, key_id(key)) << 32) | (uint64_t)(0xffffffffu - i)) : 0ull;
    }
    block_bitonic_desc<kGMergeBlock>(b, nsort, tid);
    const uint32_t m = gv.per_group;
    for (uint32_t i = tid; i < nsort; i += kGMergeBlock) {
        const uint64_t v = b[i];
        const uint32_t grp = (uint32_t)(v >> 32);
        // images before a non-empty one are non-empty (empty = 0 sorts last)
        if (v && grp != kNoGroup && i >= m && (uint32_t)(b[i - m] >> 32) == grp) a[0xffffffffu - (uint32_t)v] = 0ull;
    }
    __syncthreads();
    // ordered compaction: thread t owns a[t * kGMergePer, +kGMergePer)
    uint64_t mine[kGMergePer];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kGMergePer; ++j) {
        const uint32_t i = (uint32_t)tid * kGMergePer + j;
        mine[j] = i < nsort ? a[i] : 0ull;
        cnt += mine[j] != 0ull;
    }
    uint32_t x = cnt;  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    uint32_t pos = x - cnt, total = 0;
    for (int w = 0; w < kGMergeBlock / 64; ++w) {
        pos += (w < wave) ? wave_tot[w] : 0u;
        total += wave_tot[w];
    }
    const bool final_pass = (ngroups == 1);
    const uint32_t kept = total < k ? total : k;
    uint64_t* const okeys = out_keys ? out_keys + ((size_t)q * ngroups + g) * k : nullptr;
#pragma unroll
    for (int j = 0; j < kGMergePer; ++j) {
        if (mine[j] == 0ull) continue;
        if (pos < k) {
            if (okeys) okeys[pos] = mine[j];
            if (final_pass) {
                if (out_cos) out_cos[(size_t)q * k + pos] = key_cos(mine[j]);
                if (out_ids) out_ids[(size_t)q * k + pos] = key_id(mine[j]);
            }
        }
        ++pos;
    }
    for (uint32_t i = kept + tid; i < k; i += kGMergeBlock) {  // the slots no survivor fills
        if (okeys) okeys[i] = 0ull;
        if (final_pass) {
            if (out_cos) out_cos[(size_t)q * k + i] = 0.0f;
            if (out_ids) out_ids[(size_t)q * k + i] = 0xffffffffu;
        }
    }
    if (final_pass && out_counts && tid == 0) out_counts[q] = kept;
}

// ---- host side ------------------------------------------------------------------------------------------

template <int J, int U, int QT>
static void launch_grouped_fast(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, const float* d_queries,
                                uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv,
                                uint64_t* d_partial, hipStream_t stream) {
    hipLaunchKernelGGL((scan_grouped_topk_kernel<J, U, QT>), dim3(plan.blocks, plan.passes), dim3(kBlock), plan.lds_bytes,
                       stream, d_corpus, n_rows, d_queries, nq, k, plan.kpad, d_dead, ids, gv, d_partial);
}

template <int J, int U>
static void launch_grouped_q(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, const float* d_queries,
                             uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv,
                             uint64_t* d_partial, hipStream_t stream) {
    switch (plan.qtile) {
        case 4: launch_grouped_fast<J, U, 4>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream); break;
        case 2: launch_grouped_fast<J, U, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream); break;
        default: launch_grouped_fast<J, U, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream); break;
    }
}

int32_t launch_scan_grouped(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim,
                            const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids,
                            const GroupView& gv, uint64_t* d_partial, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    if (plan.lds_bytes > kGroupedLdsBudget || plan.kpad < k)
        return fail(CS_ERR_BAD_ARG, "grouped scan plan does not fit: %zu B of LDS, kpad %u for k %u", plan.lds_bytes, plan.kpad, k);
    if (n_rows == 0) {  // nothing to score: all-empty lists
        CS_HIP(hipMemsetAsync(d_partial, 0, plan.partial_keys * sizeof(uint64_t), stream));
        return CS_OK;
    }
    if (plan.deep && plan.qtile == 1 && grouped_fast_dim(dim)) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_grouped_fast<3, 8, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
        else if (dim == 768) launch_grouped_fast<6, 4, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
        else launch_grouped_fast<8, 3, 1>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
    } else if (dim == 384) launch_grouped_q<3, 4>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
    else if (dim == 768) launch_grouped_q<6, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
    else if (dim == 1024) launch_grouped_q<8, 2>(plan, d_corpus, n_rows, d_queries, nq, k, d_dead, ids, gv, d_partial, stream);
    else
        hipLaunchKernelGGL(scan_grouped_generic_kernel, dim3(plan.blocks, nq), dim3(kBlock), plan.lds_bytes, stream, d_corpus,
                           n_rows, dim, d_queries, nq, k, plan.kpad, d_dead, ids, gv, d_partial);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_merge_grouped(const GroupedPlan& plan, const uint64_t* d_lists, uint32_t nq, uint32_t k, const GroupView& gv,
                             uint64_t* d_tmp_a, uint64_t* d_tmp_b, uint64_t* d_out_keys, float* d_out_cos,
                             uint32_t* d_out_ids, uint32_t* d_out_counts, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    const uint32_t G = plan.merge_group;
    if (G < 2 || (uint64_t)G * k > kGroupedMergeCap)
        return fail(CS_ERR_BAD_ARG, "grouped merge takes at most %u keys per block", kGroupedMergeCap);
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(merge_topk_grouped_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kGroupedMergeCap * sizeof(uint64_t)));
        return CS_OK;
    }));
    const uint64_t* in = d_lists;
    uint64_t* bufs[2] = {d_tmp_a, d_tmp_b};
    int flip = 0;
    uint32_t nlists = plan.lists;
    for (;;) {
        const uint32_t ngroups = (nlists + G - 1) / G;
        const bool final_pass = ngroups == 1;
        uint64_t* out = final_pass ? d_out_keys : bufs[flip];
        if (!final_pass && !out) return fail(CS_ERR_BAD_ARG, "merge scratch missing");
        const uint32_t take = nlists < G ? nlists : G;
        uint32_t nsort = 64;
        while (nsort < take * k) nsort <<= 1;
        hipLaunchKernelGGL(merge_topk_grouped_kernel, dim3(ngroups, nq), dim3(kGMergeBlock), (size_t)2 * nsort * sizeof(uint64_t),
                           stream, in, nlists, k, G, (uint64_t)nlists * k, gv, out, d_out_cos, d_out_ids, d_out_counts);
        CS_HIP(hipGetLastError());
        if (final_pass) break;
        in = out;
        nlists = ngroups;
        flip ^= 1;
    }
    return CS_OK;
}


// The kernels below follow everything above so that the code of the kernels above stays, byte for byte, what it was
// before they existed (benchmarks/compare_device_code.py; profiles/grouped_scoped_device_code.log).

// ---- 1b. gathered capped scan --------------------------------------------------------------------------
// scan_grouped_topk_kernel over a row list (a scope's: live rows only, ascending, its length on the device), read as
// scan_masked_topk_kernel (scan_masked.hip) reads it: half-wave h of tile t takes row rows[t * 2U + 2u + h].  No tombstone
// test; the id is row_ids.of(row), the group group_of(gv, id).  On the slow path the row number belongs to a half-wave,
// so it is taken from the winning lane.
template <int J, int U, int QT>
__global__ void __launch_bounds__(kBlock)
scan_grouped_list_topk_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                              const uint32_t* __restrict__ rows_len, const float* __restrict__ queries, uint32_t nq,
                              uint32_t k, uint32_t kpad, RowIds row_ids, GroupView gv, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)QT * kWaves * kpad);
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;
    const uint64_t n_list = *rows_len;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }

    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi)
        qmag[qi] = load_query_fragment<J>(queries, (q0 + qi < nq) ? (q0 + qi) : (nq - 1), l32, qf[qi]);
    float thr[QT];
    uint32_t wpos[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        thr[qi] = -__builtin_huge_valf();
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
            e = e < n_list ? e : n_list - 1;  // tail entries re-read the last row, masked below
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
                if (m) {  // wave-uniform slow path; half 0 (the lower list entry, the lower id) first
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    volatile uint32_t* glist = lds_groups + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float cc = __shfl(c, src, 64);
                        const uint32_t rr = __shfl(row[u], src, 64);
                        if (cc > thr[qi]) {
                            const uint32_t id = row_ids.of(rr);
                            wave_list_insert_grouped(list, glist, k, gv.per_group, lane, cc, id, group_of(gv, id), thr[qi],
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

// Any other dim: one wave per list entry, lanes stride over columns (wave_row_cosine, scan_wave.hpp).  A template of one
// instantiation: the compiler emits instantiations behind the plain kernels of this file, in the order their launchers
// name them, so this kernel does not renumber the labels of the ones above.
template <int ROWS = 1>  // list entries in flight per wave
__global__ void __launch_bounds__(kBlock)
scan_grouped_list_generic_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                                 const uint32_t* __restrict__ rows_len, uint32_t dim, const float* __restrict__ queries,
                                 uint32_t nq, uint32_t k, uint32_t kpad, RowIds row_ids, GroupView gv,
                                 uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad] keys, then as many u32 groups
    uint32_t* const lds_groups = reinterpret_cast<uint32_t*>(lds_keys + (size_t)kWaves * kpad);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    static_assert(ROWS == 1, "one list entry in flight per wave");
    const uint32_t q = blockIdx.y;
    const uint64_t n_list = *rows_len;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) {
        lds_keys[i] = 0ull;
        lds_groups[i] = kNoGroup;
    }
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    float thr = -__builtin_huge_valf();
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    volatile uint32_t* glist = lds_groups + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t e = gw; e < n_list; e += nw) {
        const uint32_t r = rows[e];
        const float c = wave_row_cosine(corpus + (uint64_t)r * dim, qp, dim, lane, qmag);
        if (c > thr) {  // wave-uniform
            const uint32_t id = row_ids.of(r);
            wave_list_insert_grouped(list, glist, k, gv.per_group, lane, c, id, group_of(gv, id), thr, wpos);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    wave_list_store(lds_keys + (size_t)wave * kpad, k, lane, partial, q, wave);
}

// ---- 3. capped variants merge ----------------------------------------------------------------------------
// The variant merge (scan.hip merge_variants_kernel) under the cap; why capped per-variant lists may be merged, and in
// levels: grouped_plan.hpp.  in = [nlists][k] capped lists of ONE search; block g takes lists [g * G, min(nlists,
// (g + 1) * G)) and writes its capped best k distinct ids to out_keys[g][k], best first; with one block the result is final
// and count, flag and the optional decoded outputs are written too.  Per block:
//   the LDS hash of merge_variants_kernel keeps the largest key of every id (open addressing, 2 * nsort slots);
//   a[] = the table's entries, back as packed keys, sorted: position = rank under (best cosine desc, id asc);
//   b[] (the table's space, which has been read out) = the (group, ~position) images, sorted, and the cut of
//         merge_topk_grouped_kernel: a key whose image has the same group per_group places earlier is zeroed in a[];
//   the survivors, still in key order, are compacted; the first k leave.
// block_select_topk is not used: it would discard, before the cap, rows that the cap promotes.
// FINAL: the level of one block, which also decodes and writes count and flag.
template <bool FINAL>
__global__ void __launch_bounds__(kGMergeBlock)
merge_variants_grouped_kernel(const uint64_t* __restrict__ in, uint32_t nlists, uint32_t k, uint32_t G, uint32_t nsort,
                              GroupView gv, uint64_t* __restrict__ out_keys, float* __restrict__ out_cos,
                              uint32_t* __restrict__ out_ids, uint32_t* __restrict__ out_count,
                              uint32_t* __restrict__ out_high_confidence, float max_distance, uint32_t top_n) {
    extern __shared__ __attribute__((aligned(16))) uint64_t a[];  // [nsort] keys, then [2 * nsort]: the table, later the images
    __shared__ uint32_t wave_tot[kGMergeBlock / 64];
    __shared__ uint32_t nuniq, confident;
    unsigned long long* const table = reinterpret_cast<unsigned long long*>(a + nsort);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x;
    const uint32_t lo = g * G;
    const uint32_t hi = (lo + G < nlists) ? lo + G : nlists;
    const uint32_t ncand = (hi - lo) * k;  // <= nsort <= kGroupedMergeCap (the launcher's G)
    const uint64_t* src = in + (size_t)lo * k;
    const uint32_t tmask = 2 * nsort - 1;
    for (uint32_t i = tid; i < 2 * nsort; i += kGMergeBlock) table[i] = 0ull;
    if (tid == 0) { nuniq = 0; confident = 0; }
    __syncthreads();
    for (uint32_t i = tid; i < ncand; i += kGMergeBlock) {
        const uint64_t key = src[i];
        if (!key) continue;
        const uint32_t id = key_id(key);
        const unsigned long long mine = ((unsigned long long)(id + 1u) << 32) | (key >> 32);  // ids stop at 2^32 - 2
        uint32_t slot = (id * 2654435761u) & tmask;
        for (;;) {  // at most ncand <= nsort of the 2 * nsort slots are ever taken: an empty one is always met
            unsigned long long cur = table[slot];
            if (cur == 0ull) cur = atomicCAS(&table[slot], 0ull, mine);
            if (cur == 0ull) break;                                              // claimed an empty slot
            if ((uint32_t)(cur >> 32) == id + 1u) { atomicMax(&table[slot], mine); break; }  // same chunk: best cosine
            slot = (slot + 1) & tmask;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < 2 * nsort; i += kGMergeBlock) {
        const unsigned long long e = table[i];
        if (e) a[atomicAdd(&nuniq, 1u)] = (e << 32) | (uint64_t)(~((uint32_t)(e >> 32) - 1u));  // back to (image, ~id)
    }
    __syncthreads();
    uint32_t ns = 64;
    while (ns < nuniq) ns <<= 1;  // nuniq <= ncand, so ns <= nsort
    for (uint32_t i = nuniq + tid; i < ns; i += kGMergeBlock) a[i] = 0ull;
    block_bitonic_desc<kGMergeBlock>(a, ns, tid);
    uint64_t* const b = a + nsort;  // the table has been read out (a block barrier since)
    for (uint32_t i = tid; i < ns; i += kGMergeBlock) {
        const uint64_t key = a[i];
        b[i] = key ? (((uint64_t)group_of(gv, key_id(key)) << 32) | (uint64_t)(0xffffffffu - i)) : 0ull;
    }
    block_bitonic_desc<kGMergeBlock>(b, ns, tid);
    const uint32_t m = gv.per_group;
    for (uint32_t i = tid; i < ns; i += kGMergeBlock) {
        const uint64_t v = b[i];
        const uint32_t grp = (uint32_t)(v >> 32);
        // images before a non-empty one are non-empty (empty = 0 sorts last)
        if (v && grp != kNoGroup && i >= m && (uint32_t)(b[i - m] >> 32) == grp) a[0xffffffffu - (uint32_t)v] = 0ull;
    }
    __syncthreads();
    // ordered compaction: thread t owns a[t * kGMergePer, +kGMergePer)
    uint64_t mine[kGMergePer];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kGMergePer; ++j) {
        const uint32_t i = (uint32_t)tid * kGMergePer + j;
        mine[j] = i < ns ? a[i] : 0ull;
        cnt += mine[j] != 0ull;
    }
    uint32_t x = cnt;  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) wave_tot[wave] = x;
    __syncthreads();
    uint32_t pos = x - cnt, total = 0;
    for (int w = 0; w < kGMergeBlock / 64; ++w) {
        pos += (w < wave) ? wave_tot[w] : 0u;
        total += wave_tot[w];
    }
    const uint32_t kept = total < k ? total : k;
    uint64_t* const okeys = out_keys ? out_keys + (size_t)g * k : nullptr;
#pragma unroll
    for (int j = 0; j < kGMergePer; ++j) {
        if (mine[j] == 0ull) continue;
        if (pos < k) {
            if (okeys) okeys[pos] = mine[j];
            if constexpr (FINAL) {
                if (out_cos) out_cos[pos] = key_cos(mine[j]);
                if (out_ids) out_ids[pos] = key_id(mine[j]);
                // mod.rs:601-611 on the reference's own scale: distance = (1 - cos) / 2 (cs_cos_to_distance)
                if (pos < top_n && (1.0f - key_cos(mine[j])) * 0.5f < max_distance) atomicAdd(&confident, 1u);
            }
        }
        ++pos;
    }
    for (uint32_t i = kept + tid; i < k; i += kGMergeBlock) {  // the slots no survivor fills
        if (okeys) okeys[i] = 0ull;
        if constexpr (FINAL) {
            if (out_cos) out_cos[i] = 0.0f;
            if (out_ids) out_ids[i] = 0xffffffffu;
        }
    }
    if constexpr (FINAL) {
        __syncthreads();
        if (tid == 0) {
            if (out_count) *out_count = kept;
            const uint32_t want = kept < top_n ? kept : top_n;
            if (out_high_confidence) *out_high_confidence = (kept > 0 && confident == want) ? 1u : 0u;
        }
    }
}

// ---- host side of 1b and 3 ------------------------------------------------------------------------------

template <int J, int U, int QT>
static void launch_grouped_list_fast(const GroupedPlan& plan, const float* d_corpus, const uint32_t* d_list, const uint32_t* d_len,
                                     const float* d_queries, uint32_t nq, uint32_t k, RowIds ids, const GroupView& gv,
                                     uint64_t* d_partial, hipStream_t stream) {
    hipLaunchKernelGGL((scan_grouped_list_topk_kernel<J, U, QT>), dim3(plan.blocks, plan.passes), dim3(kBlock), plan.lds_bytes,
                       stream, d_corpus, d_list, d_len, d_queries, nq, k, plan.kpad, ids, gv, d_partial);
}

template <int J, int U>
static void launch_grouped_list_q(const GroupedPlan& plan, const float* d_corpus, const uint32_t* d_list, const uint32_t* d_len,
                                  const float* d_queries, uint32_t nq, uint32_t k, RowIds ids, const GroupView& gv,
                                  uint64_t* d_partial, hipStream_t stream) {
    switch (plan.qtile) {
        case 4: launch_grouped_list_fast<J, U, 4>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, d_partial, stream); break;
        case 2: launch_grouped_list_fast<J, U, 2>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, d_partial, stream); break;
        default: launch_grouped_list_fast<J, U, 1>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, gv, d_partial, stream); break;
    }
}

int32_t launch_scan_grouped_list(const GroupedPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const GroupView& gv, uint64_t* d_partial, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    if (plan.lds_bytes > kGroupedLdsBudget || plan.kpad < k)
        return fail(CS_ERR_BAD_ARG, "grouped scan plan does not fit: %zu B of LDS, kpad %u for k %u", plan.lds_bytes, plan.kpad, k);
    if (!d_list || !d_list_len) return fail(CS_ERR_BAD_ARG, "row list missing");
    if (plan.deep && plan.qtile == 1 && grouped_fast_dim(dim)) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_grouped_list_fast<3, 8, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
        else if (dim == 768) launch_grouped_list_fast<6, 4, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
        else launch_grouped_list_fast<8, 3, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
    } else if (dim == 384) launch_grouped_list_q<3, 4>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
    else if (dim == 768) launch_grouped_list_q<6, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
    else if (dim == 1024) launch_grouped_list_q<8, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, gv, d_partial, stream);
    else
        hipLaunchKernelGGL(scan_grouped_list_generic_kernel<1>, dim3(plan.blocks, nq), dim3(kBlock), plan.lds_bytes, stream,
                           d_corpus, d_list, d_list_len, dim, d_queries, nq, k, plan.kpad, ids, gv, d_partial);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_merge_variants_grouped(const uint64_t* d_keys, uint32_t nv, uint32_t k, const GroupView& gv, uint64_t* d_tmp_a,
                                      uint64_t* d_tmp_b, uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                                      uint32_t* d_out_count, uint32_t* d_out_high_confidence, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    if (!d_keys || nv == 0 || nv > CS_MAX_VARIANTS || k == 0 || k > CS_MAX_K)
        return fail(CS_ERR_BAD_ARG, "bad variant-merge arguments");
    const uint32_t G = grouped_merge_group(k);  // G * k <= kGroupedMergeCap for k <= CS_MAX_K
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(merge_variants_grouped_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 3 * kGroupedMergeCap * sizeof(uint64_t)));
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(merge_variants_grouped_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 3 * kGroupedMergeCap * sizeof(uint64_t)));
        return CS_OK;
    }));
    const uint64_t* in = d_keys;
    uint64_t* bufs[2] = {d_tmp_a, d_tmp_b};
    int flip = 0;
    uint32_t nlists = nv;
    for (;;) {
        const uint32_t ngroups = (nlists + G - 1) / G;
        const bool final_pass = ngroups == 1;
        uint64_t* out = final_pass ? d_out_keys : bufs[flip];
        if (!final_pass && !out) return fail(CS_ERR_BAD_ARG, "merge scratch missing");
        const uint32_t take = nlists < G ? nlists : G;
        uint32_t nsort = 64;
        while (nsort < take * k) nsort <<= 1;
        const size_t lds = (size_t)3 * nsort * sizeof(uint64_t);
        if (final_pass)
            hipLaunchKernelGGL(merge_variants_grouped_kernel<true>, dim3(1), dim3(kGMergeBlock), lds, stream, in, nlists, k, G,
                               nsort, gv, out, d_out_cos, d_out_ids, d_out_count, d_out_high_confidence, 0.15f, 5u);
        else
            hipLaunchKernelGGL(merge_variants_grouped_kernel<false>, dim3(ngroups), dim3(kGMergeBlock), lds, stream, in, nlists,
                               k, G, nsort, gv, out, nullptr, nullptr, nullptr, nullptr, 0.15f, 5u);
        CS_HIP(hipGetLastError());
        if (final_pass) break;
        in = out;
        nlists = ngroups;
        flip ^= 1;
    }
    return CS_OK;
}

}  // namespace cs
