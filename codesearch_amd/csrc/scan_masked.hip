// scan_masked.hip — the masked search: an exact top-k over the live rows whose chunk id a caller's bitmap allows (the
// exact form of the reference's filter_path, which post-filters a fixed candidate list: src/mcp/mod.rs:251-252,400-425,
// src/search/mod.rs:700-790).  Host plan: masked_plan.hpp.
//
//   1. row list: one pass decides, per stored row, allowed = bit(id) && id < allow_bits && !dead, and compacts the allowed
//      rows into a list in ASCENDING row order — per-block counts, one exclusive scan, a scatter.  No atomic append: the
//      per-wave lists of the scan resolve a tie with the worst slot in favour of the row already there (wave_list_insert),
//      which is the (cosine desc, id asc) order only while every wave meets its rows in ascending id.
//   2. gathered scan: scan_topk_kernel's tile loop with one change, half-wave h of tile t reads row
//      list[t * 2U + 2u + h] instead of t * 2U + 2u + h.  A row is scored by the functions that score it in the streaming
//      scan (scan_wave.hpp: load_query_fragment, row_products, cosine_of) and enters a list through the same
//      wave_list_insert, so every cosine is bit-identical to the one the full scan computes for that row, and the
//      per-block partial lists (block_merge_store) go through the same launch_merge.  Other dims: one wave per row,
//      wave_row_cosine.  (One instantiation, <8,2,4>, carries those three functions' lines as its own text: kOwnText.)
//   3. prime pass (PRIME): the streaming scan's (prime_pass_tail), over the first entries of the list.
//   4. a scope (index.hip cs_scope) keeps its row list on the device and makes it from its id list, not from a bitmap:
//      the end of this file.  Steps 2 and 3 read it as they read a mask's list.
// The list holds live rows only, so the scan tests no tombstones.
#include "scan.hpp"
#include "masked_plan.hpp"
#include "scoped_filter_plan.hpp"
#include "scan_wave.hpp"

namespace cs {

constexpr uint32_t kMaskIters = kMaskRowsPerBlock / kBlock;
static_assert(kMaskRowsPerBlock % kBlock == 0, "a row-list block decides whole 256-row steps");

// ---- 1. row list -------------------------------------------------------------------------------

__device__ __forceinline__ bool row_allowed(const uint32_t* __restrict__ allow, uint64_t lo, uint64_t hi,
                                            const uint32_t* __restrict__ dead, RowIds ids, uint64_t r) {
    const uint64_t id = ids.of(r);
    if (id < lo || id >= hi) return false;
    const uint64_t b = id - lo;
    if (!((allow[b >> 5] >> (b & 31)) & 1u)) return false;
    return !row_is_dead(dead, r);
}

// blocks[b] = allowed rows of rows [b * kMaskRowsPerBlock, +kMaskRowsPerBlock)
__global__ void __launch_bounds__(kBlock)
mask_count_kernel(const uint32_t* __restrict__ allow, uint64_t lo, uint64_t hi, const uint32_t* __restrict__ dead,
                  RowIds ids, uint64_t n_rows, uint32_t* __restrict__ blocks) {
    __shared__ uint32_t wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * kMaskRowsPerBlock;
    uint32_t c = 0;
    for (uint32_t i = 0; i < kMaskIters; ++i) {
        const uint64_t r = r0 + (uint64_t)i * kBlock + tid;
        const bool p = r < n_rows && row_allowed(allow, lo, hi, dead, ids, r);
        c += (uint32_t)__popcll(__ballot(p));
    }
    if (lane == 0) wave_cnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kWaves; ++w) s += wave_cnt[w];
        blocks[blockIdx.x] = s;
    }
}

// blocks[0, nb) -> their exclusive prefix sums; blocks[nb] = the total.  One block.
__global__ void __launch_bounds__(1024)
mask_scan_kernel(uint32_t* __restrict__ blocks, uint32_t nb) {
    __shared__ uint32_t part[1024 / 64];
    __shared__ uint32_t carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 1024) {
        const uint32_t i = base + tid;
        const uint32_t v = i < nb ? blocks[i] : 0u;
        // inclusive scan inside the wave
        uint32_t x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) part[wave] = x;
        __syncthreads();
        uint32_t before = carry;
        for (int w = 0; w < wave; ++w) before += part[w];
        if (i < nb) blocks[i] = before + x - v;
        __syncthreads();
        if (tid == 1023) carry = before + x;
        __syncthreads();
    }
    if (tid == 0) blocks[nb] = carry;
}

// list[blocks[b] + j] = the j-th allowed row of block b, ascending; never past list_cap
__global__ void __launch_bounds__(kBlock)
mask_scatter_kernel(const uint32_t* __restrict__ allow, uint64_t lo, uint64_t hi, const uint32_t* __restrict__ dead,
                    RowIds ids, uint64_t n_rows, const uint32_t* __restrict__ blocks, uint32_t* __restrict__ list,
                    uint64_t list_cap) {
    __shared__ uint32_t wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t r0 = (uint64_t)blockIdx.x * kMaskRowsPerBlock;
    uint64_t pos = blocks[blockIdx.x];
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));  // lanes under this one
    for (uint32_t i = 0; i < kMaskIters; ++i) {
        const uint64_t r = r0 + (uint64_t)i * kBlock + tid;
        const bool p = r < n_rows && row_allowed(allow, lo, hi, dead, ids, r);
        const uint64_t b = __ballot(p);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            off += (w < wave) ? wave_cnt[w] : 0u;
            total += wave_cnt[w];
        }
        const uint64_t at = pos + off + (uint32_t)__popcll(b & below);
        if (p && at < list_cap) list[at] = (uint32_t)r;
        pos += total;
        __syncthreads();  // wave_cnt is rewritten by the next step
    }
}

int32_t launch_mask_rows(const uint32_t* d_allow, uint64_t allow_lo, uint64_t allow_hi, const uint32_t* d_dead,
                         RowIds ids, uint64_t n_rows, uint32_t* d_blocks, uint32_t* d_list, uint64_t list_cap,
                         hipStream_t stream) {
    const uint32_t nb = mask_list_blocks(n_rows);
    if (nb == 0) {
        CS_HIP(hipMemsetAsync(d_blocks, 0, sizeof(uint32_t), stream));
        return CS_OK;
    }
    hipLaunchKernelGGL(mask_count_kernel, dim3(nb), dim3(kBlock), 0, stream, d_allow, allow_lo, allow_hi, d_dead, ids,
                       n_rows, d_blocks);
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, stream, d_blocks, nb);
    hipLaunchKernelGGL(mask_scatter_kernel, dim3(nb), dim3(kBlock), 0, stream, d_allow, allow_lo, allow_hi, d_dead, ids,
                       n_rows, d_blocks, d_list, list_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// mask_scan_kernel for another two-pass compaction (scope_ops.hip): any nb, totals modulo 2^32.
int32_t launch_mask_scan(uint32_t* d_blocks, uint32_t nb, hipStream_t stream) {
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, stream, d_blocks, nb);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// ---- 2. gathered scan ----------------------------------------------------------------------------
// scan_topk_kernel (scan.hip) over the list: see there for J, U, QT and the PRIME mode.
template <int J, int U, int QT, bool PRIME = false>
__global__ void __launch_bounds__(kBlock)
scan_masked_topk_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                        const uint32_t* __restrict__ rows_len, uint64_t prime_rows,
                        const float* __restrict__ queries, uint32_t nq, uint32_t k, uint32_t kpad, RowIds row_ids,
                        uint64_t* __restrict__ partial, const float* __restrict__ floor_in,
                        float* __restrict__ wave_max, uint32_t* __restrict__ done_ctr, float* __restrict__ floor_out) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [QT][kWaves][kpad]
    constexpr int DIM = 128 * J;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int half = lane >> 5;
    const int l32 = lane & 31;
    const uint32_t q0 = blockIdx.y * QT;
    uint64_t n_list = *rows_len;
    if (PRIME && n_list > prime_rows) n_list = prime_rows;

    for (uint32_t i = tid; i < QT * kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;

    // 1,024-d, four queries per pass, not the prime pass: this ONE instantiation carries the lines of load_query_fragment,
    // row_products and cosine_of as its own text.  Through the functions the compiler makes it 204 instructions shorter and
    // 0.5 - 0.9 % slower over short row lists (profiles/scan_shared_body.log); with all three inline here it is the code it
    // was before the functions existed.  The arithmetic is theirs, line for line.
    constexpr bool kOwnText = J == 8 && QT == 4 && !PRIME;
    f32x4 qf[QT][J];  // a pass past the last query re-reads query nq - 1 (its results are never stored)
    float qmag[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        const uint32_t q = (q0 + qi < nq) ? (q0 + qi) : (nq - 1);
        if constexpr (kOwnText) {
            const f32x4* qp = reinterpret_cast<const f32x4*>(queries + (size_t)q * DIM) + l32;
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                qf[qi][j] = qp[j * 32];
                s = fmaf(qf[qi][j].x, qf[qi][j].x, s);
                s = fmaf(qf[qi][j].y, qf[qi][j].y, s);
                s = fmaf(qf[qi][j].z, qf[qi][j].z, s);
                s = fmaf(qf[qi][j].w, qf[qi][j].w, s);
            }
            qmag[qi] = sqrtf(half_allreduce_sum(s));
        } else {
            qmag[qi] = load_query_fragment<J>(queries, q, l32, qf[qi]);
        }
    }
    float thr[QT], floor[QT];
    uint32_t wpos[QT];
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        floor[qi] = (!PRIME && floor_in) ? floor_in[(q0 + qi < nq) ? (q0 + qi) : (nq - 1)] : -__builtin_huge_valf();
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
            e = e < n_list ? e : n_list - 1;  // tail entries re-read the last row, masked below
            row[u] = rows[e];
            const f32x4* p = reinterpret_cast<const f32x4*>(corpus + (uint64_t)row[u] * DIM) + l32;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if constexpr (PRIME) x[u][j] = p[j * 32];  // cached: the full scan re-reads these rows right after
                else x[u][j] = __builtin_nontemporal_load(p + j * 32);
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float dot[QT];
            float xmag;
            if constexpr (kOwnText) {
                float ss = 0.0f;
#pragma unroll
                for (int qi = 0; qi < QT; ++qi) dot[qi] = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    const f32x4 v = x[u][j];
                    ss = fmaf(v.x, v.x, ss);
                    ss = fmaf(v.y, v.y, ss);
                    ss = fmaf(v.z, v.z, ss);
                    ss = fmaf(v.w, v.w, ss);
#pragma unroll
                    for (int qi = 0; qi < QT; ++qi) {
                        dot[qi] = fmaf(v.x, qf[qi][j].x, dot[qi]);
                        dot[qi] = fmaf(v.y, qf[qi][j].y, dot[qi]);
                        dot[qi] = fmaf(v.z, qf[qi][j].z, dot[qi]);
                        dot[qi] = fmaf(v.w, qf[qi][j].w, dot[qi]);
                    }
                }
                xmag = sqrtf(half_allreduce_sum(ss));
            } else {
                xmag = row_products<J, QT>(x[u], qf, dot);
            }
            const bool valid = e0 + 2 * u + half < n_list;
#pragma unroll
            for (int qi = 0; qi < QT; ++qi) {
                const float d = half_allreduce_sum(dot[qi]);
                float c;
                if constexpr (kOwnText) c = (qmag[qi] == 0.0f || xmag == 0.0f) ? 0.0f : d / (qmag[qi] * xmag);
                else c = cosine_of(d, qmag[qi], xmag);
                if constexpr (PRIME) {
                    if (valid && c > thr[qi]) thr[qi] = c;
                    continue;
                }
                unsigned long long m = __ballot(valid && l32 == 0 && c > thr[qi]);
                if (m) {  // rare: wave-uniform slow path; half 0 (the lower list entry) first
                    volatile uint64_t* list = lds_keys + ((size_t)qi * kWaves + wave) * kpad;
                    while (m) {
                        const int src = __ffsll((long long)m) - 1;
                        m &= m - 1;
                        const float cc = __shfl(c, src, 64);
                        const uint32_t rr = __shfl(row[u], src, 64);
                        if (cc > thr[qi]) wave_list_insert(list, k, lane, cc, row_ids.of(rr), thr[qi], wpos[qi], floor[qi]);
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
    const uint32_t nsort = kWaves * kpad;
#pragma unroll 1
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= nq) break;
        block_merge_store(lds_keys + (size_t)qi * nsort, kpad, k, q0 + qi, tid, partial);
    }
}

// Any other dim: one wave per list entry, lanes stride over columns (wave_row_cosine, scan_wave.hpp).
__global__ void __launch_bounds__(kBlock)
scan_masked_generic_kernel(const float* __restrict__ corpus, const uint32_t* __restrict__ rows,
                           const uint32_t* __restrict__ rows_len, uint32_t dim, const float* __restrict__ queries,
                           uint32_t nq, uint32_t k, uint32_t kpad, RowIds row_ids, uint64_t* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) uint64_t lds_keys[];  // [kWaves][kpad]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t q = blockIdx.y;
    const uint64_t n_list = *rows_len;
    for (uint32_t i = tid; i < kWaves * kpad; i += kBlock) lds_keys[i] = 0ull;
    const float* qp = queries + (size_t)q * dim;
    const float qmag = wave_query_mag(qp, dim, lane);
    float thr = -__builtin_huge_valf();
    uint32_t wpos = 0;
    __syncthreads();
    volatile uint64_t* list = lds_keys + (size_t)wave * kpad;
    const uint64_t gw = (uint64_t)blockIdx.x * kWaves + wave;
    const uint64_t nw = (uint64_t)gridDim.x * kWaves;
    for (uint64_t e = gw; e < n_list; e += nw) {
        const uint32_t r = rows[e];
        const float* xp = corpus + (uint64_t)r * dim;
        const float c = wave_row_cosine(xp, qp, dim, lane, qmag);
        if (c > thr) wave_list_insert(list, k, lane, c, row_ids.of(r), thr, wpos);  // wave-uniform
    }
    __syncthreads();
    block_merge_store(lds_keys, kpad, k, q, tid, partial);
}

template <int J, int U, int QT>
static void launch_masked_fast(const ScanPlan& plan, const float* d_corpus, const uint32_t* d_list,
                               const uint32_t* d_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                               uint64_t* d_partial, const ScanPrime* prime, bool prime_pass, uint64_t prime_rows,
                               hipStream_t stream) {
    const size_t lds = (size_t)QT * kWaves * plan.kpad * sizeof(uint64_t);
    dim3 grid(plan.blocks, plan.passes);
    if (prime_pass)
        hipLaunchKernelGGL((scan_masked_topk_kernel<J, U, QT, true>), grid, dim3(kBlock), lds, stream, d_corpus, d_list,
                           d_len, prime_rows, d_queries, nq, k, plan.kpad, ids, nullptr, nullptr, prime->d_wave_max,
                           prime->d_done, prime->d_floor);
    else
        hipLaunchKernelGGL((scan_masked_topk_kernel<J, U, QT>), grid, dim3(kBlock), lds, stream, d_corpus, d_list, d_len,
                           (uint64_t)0, d_queries, nq, k, plan.kpad, ids, d_partial, prime ? prime->d_floor : nullptr,
                           nullptr, nullptr, nullptr);
}

template <int J, int U>
static void launch_masked_q(const ScanPlan& plan, const float* d_corpus, const uint32_t* d_list, const uint32_t* d_len,
                            const float* d_queries, uint32_t nq, uint32_t k, RowIds ids, uint64_t* d_partial,
                            const ScanPrime* prime, bool prime_pass, uint64_t prime_rows, hipStream_t stream) {
    switch (plan.qtile) {
        case 4: launch_masked_fast<J, U, 4>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream); break;
        case 2: launch_masked_fast<J, U, 2>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream); break;
        default: launch_masked_fast<J, U, 1>(plan, d_corpus, d_list, d_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream); break;
    }
}

int32_t launch_scan_masked(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                           const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                           uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime, bool prime_pass,
                           uint64_t prime_rows) {
    const bool fast = dim == 384 || dim == 768 || dim == 1024;
    if (prime_pass && (!prime || !fast || prime_rows == 0))
        return fail(CS_ERR_BAD_ARG, "prime pass needs a 384/768/1024-d corpus, a sample and its buffers");
    if (plan.deep && plan.qtile == 1) {  // the streaming scan's deep shapes (scan.hip scan_deep)
        if (dim == 384) launch_masked_fast<3, 8, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
        else if (dim == 768) launch_masked_fast<6, 4, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
        else launch_masked_fast<8, 3, 1>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
    } else if (dim == 384) launch_masked_q<3, 4>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
    else if (dim == 768) launch_masked_q<6, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
    else if (dim == 1024) launch_masked_q<8, 2>(plan, d_corpus, d_list, d_list_len, d_queries, nq, k, ids, d_partial, prime, prime_pass, prime_rows, stream);
    else {
        const size_t lds = (size_t)kWaves * plan.kpad * sizeof(uint64_t);
        hipLaunchKernelGGL(scan_masked_generic_kernel, dim3(plan.blocks, nq), dim3(kBlock), lds, stream, d_corpus, d_list,
                           d_list_len, dim, d_queries, nq, k, plan.kpad, ids, d_partial);
    }
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// ---- 4. row list of a scope ----------------------------------------------------------------------
// The same list made from a scope's ascending chunk ids instead of a bitmap over the stored rows: one thread per id
// decides its row, and the survivors are compacted with the discipline of part 1 (per-block counts over
// kMaskRowsPerBlock ids, mask_scan_kernel, a ballot-ordered scatter), so ascending ids give ascending rows and the work
// follows the scope's size.  Lane l of a step reads ids[... + l]: one coalesced 256-byte read per wave.  On a compacted
// index the row comes from a lower bound over the ascending row -> id table: ~log2(n_rows) dependent loads per id.  The
// expectation behind leaving it a plain bisection (reasoning, not a measurement: the pass has not been timed on a large
// compacted index) is that neighbouring lanes hold neighbouring ids and walk the same upper levels, so those loads hit
// in cache after the first lane's miss, and that sixteen independent steps per thread at full occupancy cover the rest.
// Both kernels decide with scope_row, as the count and the scatter of part 1 both decide with row_allowed.
constexpr uint32_t kNoRow = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t scope_row(uint32_t id, const uint32_t* __restrict__ dead, RowIds ids, uint64_t n_rows) {
    uint64_t r;
    if (!ids.ids) {  // never compacted: row = id - id_base
        if (id < ids.base) return kNoRow;
        r = (uint64_t)id - ids.base;
        if (r >= n_rows) return kNoRow;  // not issued (yet)
    } else {
        uint64_t lo = 0, hi = n_rows;  // first row whose id is >= id
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (ids.ids[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (lo >= n_rows || ids.ids[lo] != id) return kNoRow;  // below id_base, not issued, or deleted and reclaimed
        r = lo;
    }
    return row_is_dead(dead, r) ? kNoRow : (uint32_t)r;
}

// blocks[b] = live rows of ids [b * kMaskRowsPerBlock, +kMaskRowsPerBlock)
__global__ void __launch_bounds__(kBlock)
scope_count_kernel(const uint32_t* __restrict__ scope_ids, uint64_t n_ids, const uint32_t* __restrict__ dead, RowIds ids,
                   uint64_t n_rows, uint32_t* __restrict__ blocks) {
    __shared__ uint32_t wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kMaskRowsPerBlock;
    uint32_t c = 0;
    for (uint32_t s = 0; s < kMaskIters; ++s) {
        const uint64_t i = i0 + (uint64_t)s * kBlock + tid;
        const bool p = i < n_ids && scope_row(scope_ids[i], dead, ids, n_rows) != kNoRow;
        c += (uint32_t)__popcll(__ballot(p));
    }
    if (lane == 0) wave_cnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int w = 0; w < kWaves; ++w) t += wave_cnt[w];
        blocks[blockIdx.x] = t;
    }
}

// list[blocks[b] + j] = the row of the j-th surviving id of block b; never past list_cap
__global__ void __launch_bounds__(kBlock)
scope_scatter_kernel(const uint32_t* __restrict__ scope_ids, uint64_t n_ids, const uint32_t* __restrict__ dead, RowIds ids,
                     uint64_t n_rows, const uint32_t* __restrict__ blocks, uint32_t* __restrict__ list, uint64_t list_cap) {
    __shared__ uint32_t wave_cnt[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t i0 = (uint64_t)blockIdx.x * kMaskRowsPerBlock;
    uint64_t pos = blocks[blockIdx.x];
    const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));  // lanes under this one
    for (uint32_t s = 0; s < kMaskIters; ++s) {
        const uint64_t i = i0 + (uint64_t)s * kBlock + tid;
        const uint32_t r = i < n_ids ? scope_row(scope_ids[i], dead, ids, n_rows) : kNoRow;
        const bool p = r != kNoRow;
        const uint64_t b = __ballot(p);
        if (lane == 0) wave_cnt[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t off = 0, total = 0;
        for (int w = 0; w < kWaves; ++w) {
            off += (w < wave) ? wave_cnt[w] : 0u;
            total += wave_cnt[w];
        }
        const uint64_t at = pos + off + (uint32_t)__popcll(b & below);
        if (p && at < list_cap) list[at] = r;
        pos += total;
        __syncthreads();  // wave_cnt is rewritten by the next step
    }
}

int32_t launch_scope_rows(const uint32_t* d_scope_ids, uint64_t n_ids, const uint32_t* d_dead, RowIds ids, uint64_t n_rows,
                          uint32_t* d_blocks, uint32_t* d_list, uint64_t list_cap, hipStream_t stream) {
    const uint32_t nb = scope_list_blocks(n_ids);
    if (nb == 0) {
        CS_HIP(hipMemsetAsync(d_blocks, 0, sizeof(uint32_t), stream));
        return CS_OK;
    }
    hipLaunchKernelGGL(scope_count_kernel, dim3(nb), dim3(kBlock), 0, stream, d_scope_ids, n_ids, d_dead, ids, n_rows,
                       d_blocks);
    hipLaunchKernelGGL(mask_scan_kernel, dim3(1), dim3(1024), 0, stream, d_blocks, nb);
    hipLaunchKernelGGL(scope_scatter_kernel, dim3(nb), dim3(kBlock), 0, stream, d_scope_ids, n_ids, d_dead, ids, n_rows,
                       d_blocks, d_list, list_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// ---- 5. what a scope keeps for the int8 filter (scoped_filter_plan.hpp) -----------------------------
// The blocked-rows bitmap is the complement of the list's bits: the launcher fills it with ones, then one thread per
// list entry clears its row's bit.  Entries are distinct, so the result does not depend on the order of the atomics.
// The same thread leaves every 1,024th entry (and the last) in the table the host reads back once per making.
__global__ void __launch_bounds__(kBlock)
scope_unblock_kernel(const uint32_t* __restrict__ list, const uint32_t* __restrict__ len, uint32_t* __restrict__ blocked,
                     uint32_t* __restrict__ table) {
    const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t n = *len;
    if (i >= n) return;
    const uint32_t r = list[i];
    atomicAnd(&blocked[r >> 5], ~(1u << (r & 31)));
    if ((i & 1023) == 0) table[1 + (i >> 10)] = r;
    if (i == n - 1) table[0] = r;
}

int32_t launch_scope_filter_state(const uint32_t* d_list, const uint32_t* d_len, uint64_t list_cap, uint64_t n_rows,
                                  uint32_t* d_blocked, uint32_t* d_table, hipStream_t stream) {
    CS_HIP(hipMemsetAsync(d_blocked, 0xFF, (size_t)scope_blocked_words(n_rows) * sizeof(uint32_t), stream));
    if (list_cap == 0) return CS_OK;
    // the list holds live rows only, so *d_len <= n_rows: threads past it have nothing to do, and a scope that names
    // more ids than the store has rows (a range of up to 2^32 - 1 ids) must not size the grid — 2^24 blocks of 256 are
    // more threads than a launch takes
    const uint64_t entries = list_cap < n_rows ? list_cap : n_rows;
    hipLaunchKernelGGL(scope_unblock_kernel, dim3((uint32_t)((entries + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                       d_list, d_len, d_blocked, d_table);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
