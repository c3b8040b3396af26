// scan_pairs.hip — the similar-pairs search (cs_index_similar_pairs): the corpus joined with itself, filter-and-refine.
//
//   filter   pairs_filter_kernel: one block per pair of 128-row tiles (ti <= tj) of the tiled f16 unit copy (scan_filter.hip:
//            [tile][k-chunk of 64][row][128 B]), a 128 x 128 x dim product on v_mfma_f32_32x32x16_f16 — BOTH operands are
//            tiles of that copy, brought in by LDS-DMA in 16-KiB stages, the staging, LDS image and swizzle of uf_mainloop
//            (scan_filter.hip; restated here so that file's text, and with it its device code, stays what it is).  On the
//            diagonal the tile is staged once and only rowA < rowB is kept.  An element not <= min_cos - margin is a
//            candidate pair (a NaN product is one: the refine decides) when both rows are stored and live and the mode
//            does not exclude the pair.
//   refine   pairs_rescore_kernel: every candidate pair re-scored from the f32 corpus, one half-wave per pair, with the
//            layout and operation order of rescore_keys_kernel (32 lanes x float4 fmaf chains, the half-wave butterfly,
//            sqrtf, the zero guard, d / (qm * xmag)); qm is formed from the lower id's row with prep_queries_kernel's
//            arithmetic.  These are the bits cs_index_search_similar gives for source a and hit b.
//
// The margin argument of scan_filter.hip carries over unchanged: both operands are the SAME unit rows rounded to f16 that
// the batched filter multiplies (there one of them is a query's unit row, prepared by the same arithmetic), the products
// are accumulated in f32 by the same instruction over the same dim terms, and filter_margin(dim) bounds |f16 product -
// exact cosine| for any two unit vectors — it never asked which side a vector came from.  The order of the k-chunks is
// rotated per block; accumulation order is one of the bound's terms.  So every pair whose exact cosine is above min_cos has
// a product above min_cos - margin and is a candidate, and a candidate's exact cosine is above min_cos - 2 margin.
#include "grouped_plan.hpp"  // kNoGroup
#include "pairs_plan.hpp"
#include "scan.hpp"
#include "split_f16.hpp"

namespace cs {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Offset (in f16 elements) of (row, k-chunk c) in the tiled filter copy — uf_tiled_off of scan_filter.hip.
__device__ __forceinline__ size_t pairs_tiled_off(uint64_t row, uint32_t c, uint32_t kchunks) {
    return (((row >> 7) * kchunks + c) * 128 + (row & 127)) * 64;
}

// The group of an id as every kernel reads the table (scan_similar.hip similar_group_of): ids past its end are ungrouped.
__device__ __forceinline__ uint32_t pairs_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

// Hits are rare and divergent: they are parked per wave in LDS (ballot + mbcnt give each its slot, as cand_push of
// scan_filter.hip does) and appended with ONE atomic per wave and batch on the single counter — one atomic per lane on one
// address serialises at the L2.  kPairsPend entries of (rowA | rowB << 32); a push adds at most 64.
constexpr uint32_t kPairsPend = 128;
typedef volatile uint64_t __attribute__((address_space(3))) pairs_lds_u64;

__device__ __forceinline__ void pairs_flush(pairs_lds_u64* pend, uint32_t& npend, int lane, uint64_t* __restrict__ cand,
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

// grid = PairsPlan::band_blocks(band_count), dynamic LDS = SH_LDS_BYTES.  Blocks b and b + 8 share an XCD's L2: XCD b & 7
// walks its own run of consecutive tile pairs — one row of the triangle at a time, so the blocks in flight on an XCD share
// the A tile and read neighbouring B tiles.
__global__ void __launch_bounds__(256, 2)
pairs_filter_kernel(const _Float16* __restrict__ corpus_h, uint32_t kchunks, uint64_t tiles, uint64_t band_first,
                    uint64_t band_count, uint64_t xcd_run, uint64_t n_rows, const uint32_t* __restrict__ dead, RowIds ids,
                    GroupView gv, int other_group, float thr, uint64_t* __restrict__ cand, unsigned long long* __restrict__ cnt,
                    uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint64_t in_band = (uint64_t)(blockIdx.x & 7) * xcd_run + (blockIdx.x >> 3);
    if (in_band >= band_count) return;
    // the buffer is already over: the call fails whatever this block finds (the host reads the counter after the band).
    // ONE thread reads the counter — it moves, and the block must take one decision: barriers follow
    if (threadIdx.x == 0)
        *reinterpret_cast<volatile uint32_t*>(lds) = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap;
    __syncthreads();
    const bool over = *reinterpret_cast<volatile uint32_t*>(lds) != 0;
    __syncthreads();  // the word is read before the first stage overwrites it
    if (over) return;
    uint64_t ti, tj;
    tile_pair_of(band_first + in_band, tiles, ti, tj);
    const bool diag = ti == tj;

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
            // rows past n_rows exist in the copy's padded last tile; they are masked at append
            asrc[i] = corpus_h + pairs_tiled_off(ti * 128 + row, 0, kchunks) + c * 8;
            wsrc[i] = corpus_h + pairs_tiled_off(tj * 128 + row, 0, kchunks) + c * 8;
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
    pairs_lds_u64* const pend = (pairs_lds_u64*)(volatile uint64_t*)(lds + wave * kPairsPend * 8);
    uint32_t npend = 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t n = wc * 64 + j * 32 + l31;
        const uint64_t rowB = tj * 128 + n;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t m = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const uint64_t rowA = ti * 128 + m;
                bool hit = !(acc[i][j][r] <= thr) && rowB < n_rows && rowA < n_rows && (!diag || m < n);
                if (!__ballot(hit)) continue;  // wave-uniform
                if (hit && dead) hit = !(((dead[rowA >> 5] >> (rowA & 31)) | (dead[rowB >> 5] >> (rowB & 31))) & 1u);
                if (hit && other_group) {  // two group reads per hit; two ungrouped chunks are never one file
                    const uint32_t ga = pairs_group_of(gv, ids.of(rowA)), gb = pairs_group_of(gv, ids.of(rowB));
                    hit = !(ga == gb && ga != kNoGroup);
                }
                const unsigned long long mask = __ballot(hit);
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                if (hit) pend[npend + before] = rowA | (rowB << 32);
                npend += (uint32_t)__popcll(mask);
                if (npend > kPairsPend - 64) pairs_flush(pend, npend, lane, cand, cnt, cap);
            }
        }
    }
    if (npend) pairs_flush(pend, npend, lane, cand, cnt, cap);
}

__device__ __forceinline__ float pairs_half_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// One half-wave per candidate pair, RU pairs per half-wave and round with their loads issued together.  A block's
// qualifying records of a round take their slots from an LDS counter and the block appends them with one atomic: the order
// of the records depends on how atomics land, the SET does not, and the caller orders it by a total order.
template <int J>
__global__ void __launch_bounds__(256)
pairs_rescore_kernel(const float* __restrict__ corpus, const uint64_t* __restrict__ cand, uint32_t n, RowIds ids,
                     float min_cos, PairRecord* __restrict__ out, uint32_t* __restrict__ total) {
    constexpr int DIM = 128 * J;
    constexpr int RU = J <= 3 ? 4 : 2;
    constexpr int PER = RU * (256 / 32);
    __shared__ uint32_t s_n, s_base;
    const int tid = threadIdx.x, l32 = tid & 31;
    const uint32_t hw = tid >> 5;
    for (uint32_t i0 = blockIdx.x * PER; i0 < n; i0 += gridDim.x * PER) {  // block-uniform
        if (tid == 0) s_n = 0;
        __syncthreads();
        uint32_t ia[RU], ib[RU], slot[RU];
        float cosv[RU];
        bool ok[RU];
        f32x4 q[RU][J], v[RU][J];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (256 / 32) + hw;  // half-wave uniform
            ok[u] = false;
            if (i < n) {
                const uint64_t e = cand[i];
                uint32_t ra = (uint32_t)e, rb = (uint32_t)(e >> 32);
                ia[u] = ids.of(ra);
                ib[u] = ids.of(rb);
                if (ia[u] > ib[u]) {  // the lower id's row is the query (rows ascend with ids: never taken today)
                    const uint32_t t = ia[u]; ia[u] = ib[u]; ib[u] = t;
                    const uint32_t s = ra; ra = rb; rb = s;
                }
                const f32x4* qp = reinterpret_cast<const f32x4*>(corpus + (size_t)ra * DIM) + l32;
                const f32x4* xp = reinterpret_cast<const f32x4*>(corpus + (size_t)rb * DIM) + l32;
#pragma unroll
                for (int j = 0; j < J; ++j) { q[u][j] = qp[j * 32]; v[u][j] = xp[j * 32]; }
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (256 / 32) + hw;
            if (i < n) {  // xor masks <= 16 stay inside the half-wave
                float s = 0.0f, ss = 0.0f, dot = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {  // prep_queries_kernel: |q|
                    s = fmaf(q[u][j].x, q[u][j].x, s); s = fmaf(q[u][j].y, q[u][j].y, s);
                    s = fmaf(q[u][j].z, q[u][j].z, s); s = fmaf(q[u][j].w, q[u][j].w, s);
                }
#pragma unroll
                for (int j = 0; j < J; ++j) {  // rescore_keys_kernel: |x| and q . x
                    ss = fmaf(v[u][j].x, v[u][j].x, ss); ss = fmaf(v[u][j].y, v[u][j].y, ss);
                    ss = fmaf(v[u][j].z, v[u][j].z, ss); ss = fmaf(v[u][j].w, v[u][j].w, ss);
                    dot = fmaf(v[u][j].x, q[u][j].x, dot); dot = fmaf(v[u][j].y, q[u][j].y, dot);
                    dot = fmaf(v[u][j].z, q[u][j].z, dot); dot = fmaf(v[u][j].w, q[u][j].w, dot);
                }
                const float qm = sqrtf(pairs_half_sum(s));
                const float xmag = sqrtf(pairs_half_sum(ss));
                const float d = pairs_half_sum(dot);
                float c = (qm == 0.0f || xmag == 0.0f) ? 0.0f : d / (qm * xmag);
                c = c + 0.0f;  // -0 -> +0, as key_pack leaves every search's cosines
                cosv[u] = c;
                // strictly above the bound; NaN / Inf cosines are never returned
                ok[u] = l32 == 0 && c > min_cos && c < __builtin_huge_valf();
                if (ok[u]) slot[u] = atomicAdd(&s_n, 1u);
            }
        }
        __syncthreads();
        if (tid == 0 && s_n) s_base = atomicAdd(total, s_n);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RU; ++u)
            if (ok[u]) out[s_base + slot[u]] = PairRecord{cosv[u], ia[u], ib[u], 0u};
    }
}

template <int J>
int32_t rescore_impl(const float* d_corpus, const uint64_t* d_cand, uint32_t n, RowIds ids, float min_cos, PairRecord* d_out,
                     uint32_t* d_total, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(pairs_rescore_kernel<J>, dim3(blocks), dim3(kPairsRefineThreads), 0, stream, d_corpus, d_cand, n, ids,
                       min_cos, d_out, d_total);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace

int32_t launch_pairs_filter(const _Float16* d_split, uint32_t dim, uint64_t tiles, uint64_t band_first, uint64_t band_count,
                            uint64_t n_rows, const uint32_t* d_dead, RowIds ids, const GroupView& gv, bool other_group,
                            float min_cos, float margin, uint64_t* d_cand, uint64_t* d_cnt, uint32_t cand_cap,
                            hipStream_t stream) {
    if (!split_scan_supported(dim)) return fail(CS_ERR_UNSUPPORTED, "similar-pairs filter: dim must be 384, 768 or 1024, got %u", dim);
    if (band_count == 0) return CS_OK;
    if (band_count > kPairsBandTilePairs || band_first + band_count > tile_pairs_of(tiles) || tiles * kPairsTileRows < n_rows)
        return fail(CS_ERR_BAD_ARG, "similar-pairs filter: band [%llu, +%llu) outside the triangle of %llu tiles",
                    (unsigned long long)band_first, (unsigned long long)band_count, (unsigned long long)tiles);
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&pairs_filter_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   SH_LDS_BYTES));
        return CS_OK;
    }));
    const uint64_t run = PairsPlan::xcd_run(band_count);
    hipLaunchKernelGGL(pairs_filter_kernel, dim3((uint32_t)PairsPlan::band_blocks(band_count)), dim3(256), SH_LDS_BYTES, stream,
                       d_split, dim / 64, tiles, band_first, band_count, run, n_rows, d_dead, ids, gv, other_group ? 1 : 0,
                       min_cos - margin, d_cand, reinterpret_cast<unsigned long long*>(d_cnt), cand_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_pairs_rescore(const float* d_corpus, uint32_t dim, const uint64_t* d_cand, uint32_t n, RowIds ids, float min_cos,
                             PairRecord* d_out, uint32_t* d_total, uint32_t blocks, hipStream_t stream) {
    if (n == 0) return CS_OK;
    switch (dim) {
        case 384: return rescore_impl<3>(d_corpus, d_cand, n, ids, min_cos, d_out, d_total, blocks, stream);
        case 768: return rescore_impl<6>(d_corpus, d_cand, n, ids, min_cos, d_out, d_total, blocks, stream);
        case 1024: return rescore_impl<8>(d_corpus, d_cand, n, ids, min_cos, d_out, d_total, blocks, stream);
        default: return fail(CS_ERR_UNSUPPORTED, "similar-pairs refine: dim must be 384, 768 or 1024, got %u", dim);
    }
}

}  // namespace cs
