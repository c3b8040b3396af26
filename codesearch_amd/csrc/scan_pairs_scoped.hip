// scan_pairs_scoped.hip — the scoped similar-pairs search (cs_index_similar_pairs_scoped): the row lists of two scopes
// joined with each other, or one with itself, filter-and-refine.  Plan: pairs_scoped_plan.hpp.
//
//   pack     pairs_pack_kernel: list entry i of a scope -> packed row i of a buffer of the call's own, the stored row's unit
//            row rounded to f16, in the filter copy's tiled layout [tile][k-chunk of 64][row][128 B].  The arithmetic is
//            unit_f16_rows_kernel's (scan_filter.hip): x / |x| in f32 from the f32 row and its stored norm, one IEEE
//            division per element, then one rounding to f16; a zero norm gives a zero row.  So the f16 bits are those the
//            index's own copy holds for that row, and THE MARGIN ARGUMENT OF scan_filter.hip's HEADER RESTS ON THIS AND ON
//            NOTHING ELSE: filter_margin(dim) bounds |f16 product - exact cosine| for two unit rows so rounded, whichever
//            buffer they sit in and at whichever position.  Rows past the list's end in the last packed tile are zeros.
//   filter   pairs_scoped_filter_kernel: pairs_filter_kernel's tile product (scan_pairs.hip: 128 x 128 x dim on
//            v_mfma_f32_32x32x16_f16, two LDS-DMA stages of 16 KiB, the LDS image and swizzle of uf_mainloop, the k-walk
//            rotated per block, 256 threads, two blocks per CU, the early `over` exit taken by one thread) — restated here
//            so that file's text, and with it its device code, stays what it is — with two operand bases and two row maps
//            (the scopes' lists) and a runtime flag: the TRIANGLE of one packed buffer (on the diagonal the tile is staged
//            once and only packed m < n is kept) or the RECTANGLE of two.  An element not <= min_cos - margin whose packed
//            rows lie below the lists' lengths is a candidate unless the mode or, in the rectangle, the duplicate rule
//            drops it; it is stored as STORED rows (lower | higher << 32) through the maps.
//   refine   launch_pairs_rescore of scan_pairs.hip, unchanged: the cosine bits are the unscoped call's by construction.
//
// The duplicate rule (rectangle only, evaluated on hits only).  The rule of the call takes each unordered pair {x, y} with
// one end in A and the other in B once.  The rectangle visits the ordered pairs (x in A, y in B).  x == y is no pair.  An
// unordered pair is visited twice exactly when both (x, y) and (y, x) are in A x B — x and y both in A and both in B —
// and then exactly one of the two visits has rA < rB: that one is kept.  Every other pair is visited once and kept.
// Membership is a binary search in the other side's ascending list.  The lists hold live rows only: no tombstone test.
#include "grouped_plan.hpp"  // kNoGroup
#include "pairs_scoped_plan.hpp"
#include "scan.hpp"
#include "split_f16.hpp"

namespace cs {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Offset (in f16 elements) of (row, k-chunk c) in the tiled filter layout — uf_tiled_off of scan_filter.hip.
__device__ __forceinline__ size_t psc_tiled_off(uint64_t row, uint32_t c, uint32_t kchunks) {
    return (((row >> 7) * kchunks + c) * 128 + (row & 127)) * 64;
}

// One thread per 8 consecutive elements of a packed row, rows [0, tiles * 128): the padding rows are written too.
__global__ void __launch_bounds__(256)
pairs_pack_kernel(const float* __restrict__ corpus, const float* __restrict__ row_norm, const uint32_t* __restrict__ list,
                  uint64_t n_list, uint64_t n8, uint32_t dim, _Float16* __restrict__ dst) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t d8 = dim / 8;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const uint64_t r = i / d8;               // packed row
        const uint32_t p = (uint32_t)(i % d8);   // 8-element piece within the row
        f16x8 o;
        if (r < n_list) {
            const uint64_t row = list[r];
            const float nrm = row_norm[row];
            const float* src = corpus + (size_t)row * dim + (size_t)p * 8;
            const f32x4 v0 = *reinterpret_cast<const f32x4*>(src);
            const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o[e] = (_Float16)(nrm == 0.0f ? 0.0f : v0[e] / nrm);
                o[4 + e] = (_Float16)(nrm == 0.0f ? 0.0f : v1[e] / nrm);
            }
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (_Float16)0.0f;
        }
        *reinterpret_cast<f16x8*>(dst + psc_tiled_off(r, p >> 3, dim / 64) + (p & 7) * 8) = o;
    }
}

__device__ __forceinline__ uint32_t psc_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

// row in list[0, n) (ascending): ceil(log2(n + 1)) + 1 reads, at most 33 (about 24 at 10M rows)
__device__ __forceinline__ bool psc_in_list(const uint32_t* __restrict__ list, uint32_t n, uint32_t row) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (list[mid] < row) lo = mid + 1;
        else hi = mid;
    }
    return lo < n && list[lo] == row;
}

// The duplicate rule's look-ups: rA is also in B's list and rB also in A's.  Not inlined: the rare path is reached from each
// of the 64 unrolled epilogue elements and would otherwise be laid out 64 times (two searches each).
__device__ __noinline__ bool psc_in_both(const uint32_t* __restrict__ listA, uint32_t nA, const uint32_t* __restrict__ listB,
                                         uint32_t nB, uint32_t rA, uint32_t rB) {
    return psc_in_list(listB, nB, rA) && psc_in_list(listA, nA, rB);
}

// Parking and flush as in scan_pairs.hip (pairs_flush): hits parked per wave in LDS, ONE atomic per wave and batch.
constexpr uint32_t kPscPend = 128;
typedef volatile uint64_t __attribute__((address_space(3))) psc_lds_u64;

__device__ __forceinline__ void psc_flush(psc_lds_u64* pend, uint32_t& npend, int lane, uint64_t* __restrict__ cand,
                                          unsigned long long* __restrict__ cnt, uint32_t cap) {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(cnt, (unsigned long long)npend);  // keeps counting past cap; stores stop at it
    base = __shfl(base, 0, 64);
    for (uint32_t i = lane; i < npend; i += 64) {
        const unsigned long long pos = base + i;
        if (pos < cap) cand[pos] = pend[i];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    npend = 0;
}

// grid = PairsPlan::band_blocks(band_count), dynamic LDS = SH_LDS_BYTES.  XCD b & 7 walks its own run of consecutive tile
// pairs: one row of the triangle or of the rectangle at a time, so the blocks in flight on an XCD share the A tile.
// tri: baseB == baseA, listB == listA, nB == nA, tiles = the side's packed tiles; else tiles = the B side's.
__global__ void __launch_bounds__(256, 2)
pairs_scoped_filter_kernel(const _Float16* __restrict__ baseA, const _Float16* __restrict__ baseB,
                           const uint32_t* __restrict__ listA, const uint32_t* __restrict__ listB, uint32_t nA, uint32_t nB,
                           uint32_t kchunks, int tri, uint64_t tiles, uint64_t band_first, uint64_t band_count,
                           uint64_t xcd_run, RowIds ids, GroupView gv, int other_group, float thr,
                           uint64_t* __restrict__ cand, unsigned long long* __restrict__ cnt, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint64_t in_band = (uint64_t)(blockIdx.x & 7) * xcd_run + (blockIdx.x >> 3);
    if (in_band >= band_count) return;
    // the buffer is already over: the call fails whatever this block finds.  ONE thread reads the moving counter, so the
    // block takes one decision: barriers follow
    if (threadIdx.x == 0)
        *reinterpret_cast<volatile uint32_t*>(lds) = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap;
    __syncthreads();
    const bool over = *reinterpret_cast<volatile uint32_t*>(lds) != 0;
    __syncthreads();  // the word is read before the first stage overwrites it
    if (over) return;
    uint64_t ti, tj;
    if (tri) tile_pair_of(band_first + in_band, tiles, ti, tj);
    else rect_pair_of(band_first + in_band, tiles, ti, tj);
    const bool diag = tri && ti == tj;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;
    sh_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    {
        const _Float16* asrc[4];
        const _Float16* wsrc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wave * 32 + i * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            // every packed tile is whole in its buffer: rows past the list's end are zeros, and masked at append
            asrc[i] = baseA + psc_tiled_off(ti * 128 + row, 0, kchunks) + c * 8;
            wsrc[i] = baseB + psc_tiled_off(tj * 128 + row, 0, kchunks) + c * 8;
        }
        auto stage = [&](uint32_t kc, char* buf) {
            char* dst = buf + wave * 32 * 128;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                sh_glds16(asrc[i] + (size_t)kc * 128 * 64, dst + i * 1024);
                if (!diag) sh_glds16(wsrc[i] + (size_t)kc * 128 * 64, dst + SH_TILE_BYTES + i * 1024);
            }
        };
        const int swz = (l31 >> 1) & 7;
        // on the diagonal the B fragments are read from the one staged tile
        const int arow = (wr * 64 + l31) * 128, wrow = (diag ? 0 : SH_TILE_BYTES) + (wc * 64 + l31) * 128;
        int sl[4];  // MFMA step s (k 16s..16s+15), lane half h -> logical 16-B slot 2s + h
#pragma unroll
        for (int s = 0; s < 4; ++s) sl[s] = ((2 * s + h) ^ swz) * 16;

        // blocks in flight on one XCD share ti and differ in tj: rotated k-walks keep them on different lines of the A tile
        uint32_t kr = (uint32_t)(tj % kchunks);
        auto next_chunk = [&]() { const uint32_t c = kr; kr = kr + 1 == kchunks ? 0 : kr + 1; return c; };
        stage(next_chunk(), lds);
        __syncthreads();
        for (uint32_t kc = 0; kc < kchunks; ++kc) {
            char* cur = lds + (kc & 1) * SH_STAGE_BYTES;
            if (kc + 1 < kchunks) stage(next_chunk(), lds + ((kc + 1) & 1) * SH_STAGE_BYTES);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                f16x8 a[2], w[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = *reinterpret_cast<const f16x8*>(cur + arow + t * 32 * 128 + sl[s]);
                    w[t] = *reinterpret_cast<const f16x8*>(cur + wrow + t * 32 * 128 + sl[s]);
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[i], w[j], acc[i][j], 0, 0, 0);
            }
            __syncthreads();
        }
    }

    // candidate <=> product > min_cos - margin, written so that NaN counts as one.  Almost every wave holds none: one
    // compare per element into a wave mask, one branch.
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) any |= __ballot(!(acc[i][j][r] <= thr));
    if (!any) return;

    // (the main loop's last barrier has retired every read of the stage buffers: the parking lists reuse them)
    psc_lds_u64* const pend = (psc_lds_u64*)(volatile uint64_t*)(lds + wave * kPscPend * 8);
    uint32_t npend = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t n = wc * 64 + j * 32 + l31;
        const uint64_t pB = tj * 128 + n;  // packed row of the B side
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t m = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const uint64_t pA = ti * 128 + m;
                bool hit = !(acc[i][j][r] <= thr) && pB < nB && pA < nA && (!diag || m < n);
                if (!__ballot(hit)) continue;  // wave-uniform
                uint32_t rA = 0, rB = 0;
                if (hit) {  // the maps are read below the lists' lengths only
                    rA = listA[pA];
                    rB = listB[pB];
                }
                if (hit && !tri) {  // the duplicate rule
                    if (rA == rB) hit = false;
                    else if (rA > rB) hit = !psc_in_both(listA, nA, listB, nB, rA, rB);
                }
                if (hit && other_group) {  // two group reads per hit; two ungrouped chunks are never one file
                    const uint32_t ga = psc_group_of(gv, ids.of(rA)), gb = psc_group_of(gv, ids.of(rB));
                    hit = !(ga == gb && ga != kNoGroup);
                }
                const unsigned long long mask = __ballot(hit);
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                if (hit) {
                    const uint64_t lo = rA < rB ? rA : rB, hi = rA < rB ? rB : rA;
                    pend[npend + before] = lo | (hi << 32);
                }
                npend += (uint32_t)__popcll(mask);
                if (npend > kPscPend - 64) psc_flush(pend, npend, lane, cand, cnt, cap);
            }
        }
    }
    if (npend) psc_flush(pend, npend, lane, cand, cnt, cap);
}

}  // namespace

int32_t launch_pairs_pack(const float* d_corpus, const float* d_norms, const uint32_t* d_list, uint64_t n_list, uint32_t dim,
                          _Float16* d_packed, hipStream_t stream) {
    if (!split_scan_supported(dim)) return fail(CS_ERR_UNSUPPORTED, "similar-pairs pack: dim must be 384, 768 or 1024, got %u", dim);
    const uint64_t n8 = packed_tiles_of(n_list) * kPairsTileRows * (dim / 8);
    if (n8 == 0) return CS_OK;
    const uint64_t want = (n8 + 255) / 256;
    hipLaunchKernelGGL(pairs_pack_kernel, dim3((uint32_t)(want < 8192 ? want : 8192)), dim3(256), 0, stream, d_corpus, d_norms,
                       d_list, n_list, n8, dim, d_packed);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_pairs_scoped_filter(const PairsScopedPlan& plan, const _Float16* d_packed_a, const _Float16* d_packed_b,
                                   const uint32_t* d_list_a, const uint32_t* d_list_b, uint32_t dim, uint64_t band_first,
                                   uint64_t band_count, RowIds ids, const GroupView& gv, bool other_group, float min_cos,
                                   float margin, uint64_t* d_cand, uint64_t* d_cnt, hipStream_t stream) {
    if (!split_scan_supported(dim)) return fail(CS_ERR_UNSUPPORTED, "similar-pairs filter: dim must be 384, 768 or 1024, got %u", dim);
    if (band_count == 0) return CS_OK;
    if (band_count > kPairsBandTilePairs || band_first + band_count > plan.tile_pairs || plan.rows_a > 0xffffffffull ||
        plan.rows_b > 0xffffffffull || plan.tiles_a * kPairsTileRows < plan.rows_a || plan.tiles_b * kPairsTileRows < plan.rows_b ||
        plan.tile_pairs != (plan.triangle ? tile_pairs_of(plan.tiles_a) : plan.tiles_a * plan.tiles_b) ||
        (plan.triangle && (d_packed_a != d_packed_b || d_list_a != d_list_b || plan.rows_a != plan.rows_b)))
        return fail(CS_ERR_BAD_ARG, "scoped similar-pairs filter: band [%llu, +%llu) outside the %s of %llu x %llu tiles",
                    (unsigned long long)band_first, (unsigned long long)band_count, plan.triangle ? "triangle" : "rectangle",
                    (unsigned long long)plan.tiles_a, (unsigned long long)plan.tiles_b);
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairs_scoped_filter_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, SH_LDS_BYTES));
        return CS_OK;
    }));
    const uint64_t run = PairsPlan::xcd_run(band_count);
    hipLaunchKernelGGL(pairs_scoped_filter_kernel, dim3((uint32_t)PairsPlan::band_blocks(band_count)), dim3(256), SH_LDS_BYTES,
                       stream, d_packed_a, d_packed_b, d_list_a, d_list_b, (uint32_t)plan.rows_a, (uint32_t)plan.rows_b, dim / 64,
                       plan.triangle ? 1 : 0, plan.triangle ? plan.tiles_a : plan.tiles_b, band_first, band_count, run, ids, gv,
                       other_group ? 1 : 0, min_cos - margin, d_cand, reinterpret_cast<unsigned long long*>(d_cnt),
                       (uint32_t)plan.cand_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
