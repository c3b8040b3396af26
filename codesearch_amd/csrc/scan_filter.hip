// scan_filter.hip — batched-query cosine scan, filter-and-refine:
//
//   filter   score_filter_kernel: [rows, dim] x [dim, Q] on the f16 MFMA (v_mfma_f32_32x32x16_f16,
//            1/16 of the exact-f32 MFMA's matrix-pipe time), 128 rows x 128 queries per block,
//            never materialised.  Both operands are the UNIT vectors x/|x| and q/|q| rounded to
//            f16 — a second, half-size copy of the corpus built at build_index (2 bytes per
//            element: the filter also reads half the bytes of the f32 scan) — so the product is
//            the cosine to within filter_margin(dim) whatever the rows' magnitudes.  An element within
//            the margin of the query's running k-th best (tau) is appended, as a row index, to that
//            query's candidate buffer.
//   refine   rescore_keys_kernel: every candidate is re-scored from the f32 corpus row with the
//            arithmetic of the single-query scan (scan.hip: 32 lanes x float4 partial fmaf
//            chains, half-wave butterfly, correctly rounded sqrt and divide), a query's rows spread
//            over up to 32 CUs;  select_candidates_kernel (scan_mfma.hip) folds the keys into the
//            running best-k, and tau becomes the exact k-th best of the rows scanned so far.
//
// Layout of the filter copy: 128-row tiles, chunk-major inside a tile — [tile][k-chunk of 64][row][128 B]
// — so the 16 KB a stage needs (one k-chunk of 128 rows) and the 96 KB of a whole tile are
// contiguous, every LDS-DMA instruction reads 1 KiB of consecutive lines, and the scan walks HBM
// sequentially (row-major rows would be visited as 128 B every 768 B, six times over).
//
// Error of the filter, for unit vectors (filter_margin() below, per model width):
//   * rounding both operands to f16: <= (2 * 2^-11 + 2^-22) * sum|q_i||x_i| <= 9.8e-4 (Cauchy-Schwarz);
//   * f32 accumulation order: <= dim * 2^-24 (2.3e-5 at 384, 6.1e-5 at 1024);
//   * elements below the f16 normal range (|v| < 2^-14): kept as f16 subnormals, absolute rounding error
//     2^-25 each, <= 2^-24 * sqrt(dim) over both operands — IF the matrix pipe consumes f16 subnormals
//     exactly, which cs_index_create checks once per device with the one-wave self-test the encoder uses
//     (sh_denorm_selftest, same v_mfma_f32_32x32x16_f16); if it ever did not, both operands' small
//     elements could be flushed: <= 2 * 2^-14 * sqrt(dim) (2.4e-3 at 384, 3.4e-3 at 768, 3.9e-3 at 1024);
//   * 2e-5 of slack for the f32 rounding of the unit vectors and of tau itself.
// Margin: 1.02e-3 / 1.05e-3 / 1.08e-3 at dim 384 / 768 / 1024 on hardware that passes the self-test
// (MI355X does), 3.4e-3 / 4.4e-3 / 5.0e-3 otherwise.  Every row whose exact cosine beats tau is therefore
// a candidate and the result equals the exact scan's bit for bit — ids and cosines.  The price of the
// margin is a handful of extra candidates per query (rows whose cosine lies within it below the k-th
// best), each one a 1.5 KB re-read.  CS_FILTER_MARGIN overrides (A/B only).
// Phases (row-ordered, growing 5x: 1 K, 5 K, 25 K ... rows) and the overflow escape hatch are those
// of scan_mfma.hip.  Serves `variants.par_iter().map(|e| store.search(e, limit))`
// (/root/reference/src/search/mod.rs:508-511) and BASELINE.json configs 4/5.
#include <array>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include <cmath>
#include "scan.hpp"
#include "split_f16.hpp"

namespace cs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// cosine units; bound derived in the header comment
float filter_margin(uint32_t dim, bool subnormals_exact) {
    static const float forced = [] {
        const char* e = cs_lab_env("CS_FILTER_MARGIN");
        return e ? (float)std::atof(e) : 0.0f;
    }();
    if (forced > 0.0f) return forced;
    const float sq = sqrtf((float)dim);
    const float small = subnormals_exact ? 5.9604645e-08f * sq : 2.0f * 6.1035156e-05f * sq;
    return 9.8e-4f + (float)dim * 5.9604645e-08f + small + 2.0e-5f;
}

// ---- candidate append, batched per wave ---------------------------------------------------------
// An append is a device-scope atomic WITH return on the query's counter: a ~2 us round trip during
// which the wave does nothing else, and at k = 200 one tile in ten holds a candidate.  So hits are
// first parked in a wave-private LDS list — ballot + mbcnt give each hit its slot, no atomics — and
// the list is appended in one go (all lanes' atomics in flight together: one round trip per batch).
// Used by the resident-query kernel, a pure HBM stream; in the MFMA-bound tile kernels the ballot per
// accumulator element costs more than the stalls it saves (100 queries 1.98 -> 2.10 ms, 1000 queries
// 9.0 -> 9.8 ms), so they append directly.
// kPend entries of (query << 32 | row); a push adds at most 64, so the list is flushed above kPend - 64.
constexpr uint32_t kPend = 128;

// The parking list is LDS and is addressed as such: through a generic pointer the accesses become flat_store /
// flat_load, which count on vmcnt too and return out of order with the corpus loads in flight, and every counted
// `s_waitcnt vmcnt(N)` of the streaming loop behind a possible push degrades to vmcnt(0).
typedef volatile uint64_t __attribute__((address_space(3))) lds_vu64;

__device__ __forceinline__ void cand_flush(volatile uint64_t* pend_generic, uint32_t& npend, int lane,
                                           uint32_t* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap) {
    lds_vu64* const pend = (lds_vu64*)pend_generic;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t i = lane; i < npend; i += 64) {
        const uint64_t e = pend[i];
        const uint32_t q = (uint32_t)(e >> 32);
        const uint32_t pos = atomicAdd(&cnt[(size_t)q * kCntStride], 1u);
        if (pos < cap) cand[2 * ((size_t)q * cap + pos)] = (uint32_t)e;  // low word of the 8-byte slot
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
    npend = 0;
}

// All 64 lanes call this together; `hit` lanes park (q, row).  Tombstoned rows are dropped here.
__device__ __forceinline__ void cand_push(bool hit, uint32_t q, uint64_t row, const uint32_t* __restrict__ dead,
                                          volatile uint64_t* pend_generic, uint32_t& npend, int lane,
                                          uint32_t* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap) {
    lds_vu64* const pend = (lds_vu64*)pend_generic;
    unsigned long long mask = __ballot(hit);
    if (!mask) return;  // wave-uniform; the common case
    if (dead) {
        if (hit) hit = !((dead[row >> 5] >> (row & 31)) & 1u);
        mask = __ballot(hit);
    }
    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    if (hit) pend[npend + before] = ((uint64_t)q << 32) | (uint32_t)row;
    npend += (uint32_t)__popcll(mask);
    if (npend > kPend - 64) cand_flush(pend_generic, npend, lane, cand, cnt, cap);
}

__device__ __forceinline__ float half_sum_s(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// int8 filter operands (section "int8 filter copy" below)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
constexpr float kQ8Half = 0.5001f, kQ8Quarter = 0.2501f, kQ8Guard = 4.0f;
__host__ __device__ __forceinline__ float q8_slack(uint32_t dim) { return (float)dim * 1.1920929e-07f + 4.0e-5f; }

__device__ __forceinline__ int half_sum_i(int v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}
__device__ __forceinline__ float half_max_q8(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 8, 64));
    v = fmaxf(v, __shfl_xor(v, 4, 64));
    v = fmaxf(v, __shfl_xor(v, 2, 64));
    v = fmaxf(v, __shfl_xor(v, 1, 64));
    return v;
}
// four unit values -> four int8 in one dword (element 0 in the low byte), and the sum of their magnitudes
// ... and of their squares (sq_sum) and of the squared rounding errors (err_sum): the Cauchy-Schwarz side of the bound
__device__ __forceinline__ uint32_t q8_pack4(const f32x4 u, float inv, int& abs_sum, float& sq_sum, float& err_sum) {
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float t = u[e] * inv;
        float r = rintf(t);
        r = fminf(fmaxf(r, -127.0f), 127.0f);  // NaN -> -127 (fmaxf drops it): such a tile is flagged anyway
        const int a = (int)r;
        abs_sum += a < 0 ? -a : a;
        sq_sum = fmaf(r, r, sq_sum);
        err_sum = fmaf(t - r, t - r, err_sum);
        w |= ((uint32_t)a & 0xffu) << (8 * e);
    }
    return w;
}
// The threshold of the int8 filter for one (tile, query): a row can beat tau only if its integer product I exceeds it.
//   tile  {inv_t, 0.5001 B_t, E_t, N_t}:  B_t / E_t / N_t = the largest sum |a_i| / error norm sqrt(sum e_i^2) / norm
//                                         sqrt(sum a_i^2) of the tile's rows
//   query tqs = (tau - slack - q.mu) inv_q,  hA = 0.5001 sum |b_i|,  nb = sqrt(sum b_i^2),  Dq = sqrt(sum d_i^2)
// |sum b_i e_i| <= min(max|e| sum|b_i|, |b| |e|) and likewise for the other two error terms: whichever side is tighter
// (the L1 side for sparse or one-hot vectors, the Cauchy-Schwarz side — ~0.7 of it — for evenly spread ones).
__device__ __forceinline__ float q8_threshold(float tqs, float hA, float nb, float Dq, const float4 tm, float dimq) {
    const float tA = fminf(hA, nb * tm.z);
    const float tB = fminf(tm.y, tm.w * Dq);
    const float tC = fminf(dimq, tm.z * Dq);
    // the f32 evaluation of the line itself: a relative term (with two-plane queries |T| reaches 1e9: an ulp is 64)
    // (capped, so that tau = +inf keeps T = +inf — nothing passes — instead of inf - inf = NaN, which passes every row)
    const float lead = tqs * tm.x;
    return floorf(lead - (tA + tB + tC + kQ8Guard + fminf(fabsf(lead) * 4.0e-7f, 3.0e38f)));
}

// Everything a batched search needs before its first phase, in one launch (three kernels of ~2 us
// each cost ~12 us of launch gaps — a quarter of a search over the reference's own 592-chunk index):
// per query, one half-wave computes |q| with the single-query scan's arithmetic (scan.hip, "query
// fragments + magnitudes"), writes q/|q| as f16 row-major (the arithmetic of unit_f16_rows_kernel)
// and resets the query's search state.
template <int J>
__global__ void __launch_bounds__(256)
prep_queries_kernel(const float* __restrict__ queries, float* __restrict__ qcopy, uint32_t nq,
                    float* __restrict__ qmag, _Float16* __restrict__ qunit, float* __restrict__ tau, uint32_t* __restrict__ cnt,
                    uint64_t* __restrict__ carry, uint32_t k, uint32_t* __restrict__ overflow, uint32_t first_rows,
                    int8_t* __restrict__ q8q, float4* __restrict__ qmeta, const float* __restrict__ mu,
                    uint32_t* __restrict__ overflow_mirror, int8_t* __restrict__ q8q_hi, int8_t* __restrict__ q8q_lo) {
    constexpr int DIM = 128 * J;
    const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    const uint32_t q = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 2 + half;
    const uint32_t qq = q < nq ? q : nq - 1;
    const f32x4* qp = reinterpret_cast<const f32x4*>(queries + (size_t)qq * DIM) + l32;
    f32x4 v[J];
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        v[j] = qp[j * 32];
        s = fmaf(v[j].x, v[j].x, s); s = fmaf(v[j].y, v[j].y, s); s = fmaf(v[j].z, v[j].z, s); s = fmaf(v[j].w, v[j].w, s);
    }
    const float m = sqrtf(half_sum_s(s));
    if (q >= nq) return;  // after the half-wave reduction
    typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
    if (qcopy) {  // queries came from pinned host memory: leave a device copy for the refine kernels
#pragma unroll
        for (int j = 0; j < J; ++j) reinterpret_cast<f32x4*>(qcopy + (size_t)q * DIM)[l32 + 32 * j] = v[j];
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        f16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (_Float16)(m == 0.0f ? 0.0f : v[j][e] / m);
        *reinterpret_cast<f16x4*>(qunit + (size_t)q * DIM + (l32 + 32 * j) * 4) = o;
    }
    if (q8q) {  // int8 filter operand ("int8 filter copy" below): q / |q| on the query's own scale
        float mx = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, fabsf(m == 0.0f ? 0.0f : v[j][e] / m));
        mx = half_max_q8(mx);
        const float inv = (mx > 0.0f && mx < __builtin_huge_valf()) ? 127.0f / mx : 1.0f;
        int abs_sum = 0;
        float sq_sum = 0.0f, err_sum = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            f32x4 u;
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = m == 0.0f ? 0.0f : v[j][e] / m;
            *reinterpret_cast<uint32_t*>(q8q + (size_t)q * DIM + (l32 + 32 * j) * 4) = q8_pack4(u, inv, abs_sum, sq_sum, err_sum);
        }
        abs_sum = half_sum_i(abs_sum);
        sq_sum = half_sum_s(sq_sum);
        err_sum = half_sum_s(err_sum);
        // the corpus copy holds u - mu (mu: the mean unit row at the first build): q.u = q.(u - mu) + q.mu, the second
        // term exact per query
        float qmu = 0.0f;
        if (mu) {
#pragma unroll
            for (int j = 0; j < J; ++j) {
                const f32x4 mv = *reinterpret_cast<const f32x4*>(mu + (l32 + 32 * j) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) qmu = fmaf(m == 0.0f ? 0.0f : v[j][e] / m, mv[e], qmu);
            }
            qmu = half_sum_s(qmu);
        }
        if (l32 == 0) {  // (norms a hair up: their own f32 rounding)
            qmeta[q] = make_float4(inv, kQ8Half * (float)abs_sum, qmu, sqrtf(sq_sum) * 1.0001f);
            qmeta[nq + q] = make_float4(sqrtf(err_sum) * 1.001f + 1.0e-3f, 0.0f, 0.0f, 0.0f);
        }
        if (q8q_hi) {
            // The same query 128 times finer, in TWO int8 planes: B_i = rint(v_i * 128 inv) = 128 hi_i + lo_i with hi in
            // [-127, 127] and lo in [-64, 64], so sum a_i B_i = 128 (a . hi) + (a . lo): two MFMAs per step, where the
            // matrix pipe has room (up to 64 queries the filter is a stream).  The query's rounding error — half the band
            // for evenly spread vectors — shrinks 128-fold; the constants below are in the finer unit.
            const float inv2 = inv * 128.0f;
            float abs2 = 0.0f, sq2 = 0.0f, err2 = 0.0f;
#pragma unroll
            for (int j = 0; j < J; ++j) {
                uint32_t whi = 0, wlo = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float t = (m == 0.0f ? 0.0f : v[j][e] / m) * inv2;
                    float B = rintf(t);
                    B = fminf(fmaxf(B, -16256.0f), 16256.0f);
                    const float hi = rintf(B * 0.0078125f);
                    const float lo = B - 128.0f * hi;   // exact: |lo| <= 64
                    abs2 += fabsf(B);
                    sq2 = fmaf(B, B, sq2);
                    err2 = fmaf(t - B, t - B, err2);
                    whi |= ((uint32_t)(int)hi & 0xffu) << (8 * e);
                    wlo |= ((uint32_t)(int)lo & 0xffu) << (8 * e);
                }
                *reinterpret_cast<uint32_t*>(q8q_hi + (size_t)q * DIM + (l32 + 32 * j) * 4) = whi;
                *reinterpret_cast<uint32_t*>(q8q_lo + (size_t)q * DIM + (l32 + 32 * j) * 4) = wlo;
            }
            abs2 = half_sum_s(abs2);
            sq2 = half_sum_s(sq2);
            err2 = half_sum_s(err2);
            if (l32 == 0) {
                qmeta[2 * nq + q] = make_float4(inv2, kQ8Half * abs2 * 1.0001f, qmu, sqrtf(sq2) * 1.0001f);
                qmeta[3 * nq + q] = make_float4(sqrtf(err2) * 1.001f + 1.0e-3f, 0.0f, 0.0f, 0.0f);
            }
        }
    }
    for (uint32_t i = l32; i < k; i += 32) carry[(size_t)q * k + i] = 0ull;
    if (l32 == 0) {
        qmag[q] = m;
        tau[q] = -__builtin_huge_valf();
        cnt[(size_t)q * kCntStride] = first_rows;
        if (q == 0) {
            overflow[2] += overflow[0];
            overflow[0] = 0;
            if (overflow_mirror) *overflow_mirror = overflow[2];
        }
    }
}

// Offset (in f16 elements) of (row, k-chunk c) in the tiled filter copy; + 8 * piece for the 16-B pieces.
__host__ __device__ __forceinline__ size_t uf_tiled_off(uint64_t row, uint32_t c, uint32_t kchunks) {
    return (((row >> 7) * kchunks + c) * 128 + (row & 127)) * 64;
}

// rows of an f32 matrix, each divided by its norm (zero norm -> zero row), as f16; one thread per 8
// consecutive elements.  tiled: destination row index dst_row0 + r in the layout above (the corpus
// copy); otherwise plain row-major [rows][dim] (the queries).
__global__ void __launch_bounds__(256)
unit_f16_rows_kernel(const float* __restrict__ src, const float* __restrict__ row_norm,
                     _Float16* __restrict__ dst, uint64_t n8, uint32_t dim, int tiled, uint64_t dst_row0) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t d8 = dim / 8;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
        const uint64_t r = i / d8;
        const uint32_t p = (uint32_t)(i % d8);  // 8-element piece within the row
        const float nrm = row_norm[r];
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(src + i * 8);
        const f32x4 v1 = *reinterpret_cast<const f32x4*>(src + i * 8 + 4);
        f16x8 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o[e] = (_Float16)(nrm == 0.0f ? 0.0f : v0[e] / nrm);
            o[4 + e] = (_Float16)(nrm == 0.0f ? 0.0f : v1[e] / nrm);
        }
        _Float16* d = tiled ? dst + uf_tiled_off(dst_row0 + r, p >> 3, dim / 64) + (p & 7) * 8 : dst + i * 8;
        *reinterpret_cast<f16x8*>(d) = o;
    }
}

// 128 x 128 x 64 tile main loop on plain f16 operands: the staging, LDS image and swizzle of
// sh_mainloop16 (split_f16.hpp) — a stage is one 128-B line per row — but the line holds 64
// consecutive k of one f16 plane, so a stage is four MFMA k-steps into ONE accumulator set.
__device__ __forceinline__ void uf_mainloop(const _Float16* __restrict__ A, uint32_t M, uint32_t m0,
                                            const _Float16* __restrict__ W, uint32_t N, uint32_t n0,
                                            uint32_t kchunks, char* lds, sh_f32x16 (&acc)[2][2], uint32_t kc_rot,
                                            bool nt_corpus) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l31 = lane & 31, h = lane >> 5;
    const _Float16* asrc[4];
    const _Float16* wsrc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = wave * 32 + i * 8 + (lane >> 3);
        const int c = (lane & 7) ^ ((row >> 1) & 7);
        // A is the tiled filter copy (rows past M exist in its padded last tile and are masked at
        // append); m0 is a multiple of 128, so the block's rows are one tile
        const uint32_t wn = (n0 + row < N) ? n0 + row : N - 1;
        asrc[i] = A + uf_tiled_off(m0 + row, 0, kchunks) + c * 8;
        wsrc[i] = W + (size_t)wn * kchunks * 64 + c * 8;
    }
    auto stage = [&](uint32_t kc, char* buf) {
        char* dst = buf + wave * 32 * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (nt_corpus) sh_glds16_nt(asrc[i] + (size_t)kc * 128 * 64, dst + i * 1024);
            else sh_glds16(asrc[i] + (size_t)kc * 128 * 64, dst + i * 1024);
            sh_glds16(wsrc[i] + (size_t)kc * 64, dst + SH_TILE_BYTES + i * 1024);
        }
    };
    const int swz = (l31 >> 1) & 7;
    const int arow = (wr * 64 + l31) * 128, wrow = SH_TILE_BYTES + (wc * 64 + l31) * 128;
    int sl[4];  // MFMA step s (k 16s..16s+15), lane half h -> logical 16-B slot 2s + h
#pragma unroll
    for (int s = 0; s < 4; ++s) sl[s] = ((2 * s + h) ^ swz) * 16;

    uint32_t kr = kc_rot % kchunks;
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

// grid = sh_grid_blocks(row tiles of the phase, query tiles); dynamic LDS = SH_LDS_BYTES.
__global__ void __launch_bounds__(256, 2)
score_filter_kernel(const _Float16* __restrict__ corpus_h, uint64_t row_lo, uint64_t row_hi, uint32_t kchunks,
                    const _Float16* __restrict__ queries_h, uint32_t nq, const float* __restrict__ tau,
                    const uint32_t* __restrict__ dead, uint32_t* __restrict__ cand, uint32_t* __restrict__ cnt,
                    uint32_t cap, float margin) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint32_t M = (uint32_t)(row_hi - row_lo);
    const uint32_t ntiles = (nq + SH_BN - 1) / SH_BN;
    uint32_t mt, nt;
    if (!sh_tile_of_block(blockIdx.x, (M + SH_BM - 1) / SH_BM, ntiles, mt, nt)) return;
    const uint32_t m0 = mt * SH_BM, n0 = nt * SH_BN;
    sh_f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
    uf_mainloop(corpus_h + uf_tiled_off(row_lo, 0, kchunks), M, m0, queries_h, nq, n0, kchunks, lds, acc,
                sh_kc_rot(nt, ntiles, kchunks), /*nt_corpus=*/ntiles == 1);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t q = n0 + wc * 64 + j * 32 + l31;
        const bool qok = q < nq;
        // candidate <=> approx_cos > tau - margin, written so that NaN (a row holding NaN/Inf)
        // counts as a candidate: refine decides
        const float tq = qok ? tau[q] - margin : 0.0f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t m = m0 + wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                if (qok && m < M && !(acc[i][j][r] <= tq)) {  // rare, divergent, short
                    const uint64_t row = row_lo + m;
                    if (!dead || !((dead[row >> 5] >> (row & 31)) & 1u)) {
                        const uint32_t pos = atomicAdd(&cnt[(size_t)q * kCntStride], 1u);
                        if (pos < cap) cand[2 * ((size_t)q * cap + pos)] = (uint32_t)row;  // low word of the 8-byte slot
                    }
                }
            }
        }
    }
}

// ---- 256 x 256 x 64 tiles for more than 128 queries -------------------------------------------
// 8 waves as 4 (rows) x 2 (queries), a wave owns 64 rows x 128 queries = 2 x 4 MFMA tiles (128
// accumulator registers): per byte staged into LDS twice the MFMA work of the 128 x 128 tile —
// the global -> LDS fill path (~10 TB/s chip-wide with operands coming partly from HBM) is what
// bounds these kernels, not the matrix pipe.  One block per CU (2 x 64 KiB stages).
constexpr int UF2_BM = 256, UF2_BN = 256, UF2_TILE = 256 * 128, UF2_STAGE = 2 * UF2_TILE, UF2_LDS = 2 * UF2_STAGE;

// ---- the 256 x 256 tiles as a persistent kernel with cross-tile prefetch ------------------------------
// dim 384 is only six 64-k stages per tile, and with one block per CU (128 KiB of LDS) nothing covers a
// tile's first stage (an HBM round trip when the corpus rows are cold) or its epilogue.  Here a block
// walks tiles b, b + grid, ... (same XCD, consecutive tile slots: the XCD-shared walk of
// sh_tile_of_block is kept) and issues stage 0 of its NEXT tile between the MFMAs of the current
// tile's last stage, into the buffer that stage leaves free; the threshold epilogue then runs under
// that load.  The wave's eight LDS-DMA instructions of the NEXT stage go out one at a time between the MFMAs of
// this one (an LDS-DMA costs its wave ~35+ cycles of issue while the CU's address path accepts it: issued back
// to back at the top of the step, with all eight waves doing the same, they hold the matrix pipe idle for about
// as long as the step's MFMAs take; see the ablation table in DESIGN.md §3.3).  Fragment reads are explicit asm
// with counted lgkmcnt, double-buffered across the sub-steps of a stage.  (The one-block-per-tile form of this
// kernel and its DMAs-at-step-start variant, rounds 1-2, are no longer built.)
//
// I8: the same kernel over the int8 copy ("int8 filter copy" above).  A 128-B line is 128 k instead of 64, the MFMA is
// v_mfma_i32_16x16x64_i8 on the same 16-B fragments — every address below is unchanged, with kchunks = dim / 128 and
// the int8 buffers passed as if they were f16 (64 two-byte elements per line) — at twice the f16 rate per matrix
// instruction.  A wave's 64 rows lie in ONE 128-row corpus tile (tile 2 mt + (wr >> 1)), so its scale is a scalar;
// `margin` carries the slack and tmeta / qmeta the scales (see score_filter_rw8_kernel for the threshold).
template <bool I8>
__global__ void __launch_bounds__(512, 2)
score_filter256p_kernel(const _Float16* __restrict__ corpus_h, uint64_t row_lo, uint64_t row_hi, uint32_t kchunks,
                        const _Float16* __restrict__ queries_h, uint32_t nq, const float* __restrict__ tau,
                        const uint32_t* __restrict__ dead, uint32_t* __restrict__ cand,
                        uint32_t* __restrict__ cnt, uint32_t cap, uint32_t total_slots, float margin,
                        const float4* __restrict__ tmeta, const float4* __restrict__ qmeta) {
    using Frag = typename std::conditional<I8, i32x4, f16x8>::type;
    using Acc = typename std::conditional<I8, i32x4, sh_f32x4v>::type;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint32_t M = (uint32_t)(row_hi - row_lo);
    const uint32_t mtiles = (M + UF2_BM - 1) / UF2_BM, ntiles = (nq + UF2_BN - 1) / UF2_BN;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int l15 = lane & 15, g = lane >> 4;  // 16x16x32 MFMA: row | query of the lane, k-group of 8
    const _Float16* A = corpus_h + uf_tiled_off(row_lo, 0, kchunks);  // row_lo is a multiple of 128

    // first live tile slot of this block at or after `slot` (slots of padding m-tiles are skipped)
    auto next_live = [&](uint32_t slot, uint32_t& mt, uint32_t& nt) {
        for (; slot < total_slots; slot += gridDim.x)
            if (sh_tile_of_block(slot, mtiles, ntiles, mt, nt)) return slot;
        return total_slots;
    };
    // per-lane source pointers of a tile's stage pieces (4 corpus pieces, 4 query pieces per wave)
    auto tile_ptrs = [&](uint32_t mt, uint32_t nt, const _Float16* (&ap)[4], const _Float16* (&wp)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wave * 32 + i * 8 + (lane >> 3);
            const int c = (lane & 7) ^ ((row >> 1) & 7);
            const uint32_t wn = (nt * UF2_BN + row < nq) ? nt * UF2_BN + row : nq - 1;
            ap[i] = A + uf_tiled_off(mt * UF2_BM + row, 0, kchunks) + c * 8;  // padded tiles: no row clamp needed
            wp[i] = queries_h + (size_t)wn * kchunks * 64 + c * 8;
        }
    };
    // v_mfma_f32_16x16x32_f16: a wave's 64 rows x 128 queries = 4 x 8 MFMA tiles; one MFMA takes 32 k of a
    // row's 128-B line (16-B piece 4s + g of k32 step s).  Same MFMA cycles and LDS bytes per flop as the
    // 32x32x16 form; the chip holds a higher clock under it (MI355X_MICROARCH.md, DVFS give-back item 7).
    // rows wr*64 + 16 i + l15 and queries wc*128 + 16 j + l15: (row >> 1) & 7 = l15 >> 1 for every i, j
    const int swz = (l15 >> 1) & 7;
    const int arow = (wr * 64 + l15) * 128, wrow = UF2_TILE + (wc * 128 + l15) * 128;
    int sl[2];
#pragma unroll
    for (int s = 0; s < 2; ++s) sl[s] = ((4 * s + g) ^ swz) * 16;
    const uint32_t lds_base = (uint32_t)(uintptr_t)lds;
    // fragments of a k32 step s: 4 corpus row groups (load_a), and 4 of the 8 query groups (load_w, qh = 0, 1)
    auto load_a = [&](uint32_t stage_off, int s, Frag (&f)[4]) {
        const uint32_t aa = lds_base + stage_off + arow + sl[s];
        asm volatile("ds_read_b128 %0, %1" : "=v"(f[0]) : "v"(aa));
        asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(f[1]) : "v"(aa));
        asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(f[2]) : "v"(aa));
        asm volatile("ds_read_b128 %0, %1 offset:6144" : "=v"(f[3]) : "v"(aa));
    };
    auto load_w = [&](uint32_t stage_off, int s, int qh, Frag (&f)[4]) {
        const uint32_t ww = lds_base + stage_off + wrow + sl[s] + qh * 8192;
        asm volatile("ds_read_b128 %0, %1" : "=v"(f[0]) : "v"(ww));
        asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(f[1]) : "v"(ww));
        asm volatile("ds_read_b128 %0, %1 offset:4096" : "=v"(f[2]) : "v"(ww));
        asm volatile("ds_read_b128 %0, %1 offset:6144" : "=v"(f[3]) : "v"(ww));
    };
#define UF2_LGKM_WAIT(N)                                           \
    do {                                                           \
        asm volatile("s_waitcnt lgkmcnt(" #N ")" ::: "memory");    \
        __builtin_amdgcn_sched_barrier(0);                         \
    } while (0)

    // one query tile: a corpus tile is read by exactly one block, once — stream it past the caches
    const bool nt_corpus = ntiles == 1;
    uint32_t mt, nt, mtn = 0, ntn = 0;
    uint32_t slot = next_live(blockIdx.x, mt, nt);
    if (slot >= total_slots) return;
    const _Float16 *a_cur[4], *w_cur[4], *a_nxt[4], *w_nxt[4];
    tile_ptrs(mt, nt, a_cur, w_cur);
    uint32_t kr = sh_kc_rot(nt, ntiles, kchunks);  // chunk of the next stage to issue for the current tile
    uint32_t par = 0;                              // buffer of the current tile's stage 0
    {   // stage 0 of the first tile
        char* dst = lds + wave * 32 * 128;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (nt_corpus) sh_glds16_nt(a_cur[i] + (size_t)kr * 128 * 64, dst + i * 1024);
            else sh_glds16(a_cur[i] + (size_t)kr * 128 * 64, dst + i * 1024);
            sh_glds16(w_cur[i] + (size_t)kr * 64, dst + UF2_TILE + i * 1024);
        }
        kr = kr + 1 == kchunks ? 0 : kr + 1;
    }
    for (;;) {
        const uint32_t slot_n = next_live(slot + gridDim.x, mtn, ntn);
        const bool have_next = slot_n < total_slots;
        uint32_t krn = 0;
        if (have_next) {
            tile_ptrs(mtn, ntn, a_nxt, w_nxt);
            krn = sh_kc_rot(ntn, ntiles, kchunks);
        }
        Acc acc[4][8];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[i][j][r] = 0;
        // sixteen MFMAs (4 row groups x 4 query groups jb..jb+3) of half a k32 step; with `issue`, DMA pieces
        // q0..q0+3 (0..3 corpus, 4..7 queries) of chunk kcn — of this tile, or of the next tile's stage 0
        // when `from_next` — after MFMAs 4, 8, 12, 16
        auto mfma16 = [&](const Frag (&fa)[4], const Frag (&fw)[4], int jb, bool issue, bool from_next, int q0,
                          uint32_t kcn, char* nbuf) {
            char* dst = nbuf + wave * 32 * 128;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if constexpr (I8) acc[i][jb + j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fw[j], acc[i][jb + j], 0, 0, 0);
                    else acc[i][jb + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(fa[i], fw[j], acc[i][jb + j], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                if (issue) {
                    const int q = q0 + j;
                    if (q < 4) {
                        const _Float16* src = (from_next ? a_nxt[q] : a_cur[q]) + (size_t)kcn * 128 * 64;
                        if (nt_corpus) sh_glds16_nt(src, dst + q * 1024);
                        else sh_glds16(src, dst + q * 1024);
                    } else {
                        sh_glds16((from_next ? w_nxt[q - 4] : w_cur[q - 4]) + (size_t)kcn * 64, dst + UF2_TILE + (q - 4) * 1024);
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        sh_wait_vmcnt<0>();             // this wave's pieces of the tile's stage 0 (and the last epilogue's stores)
        __builtin_amdgcn_s_barrier();   // ... and everybody else's
        __builtin_amdgcn_sched_barrier(0);
        Frag a0[4], a1[4], w0[4], w1[4];
        load_a(par * UF2_STAGE, 0, a0);
        load_w(par * UF2_STAGE, 0, 0, w0);
        for (uint32_t kc = 0; kc < kchunks; ++kc) {
            const uint32_t b = (par + kc) & 1;
            const uint32_t so = b * UF2_STAGE;
            char* nbuf = lds + (b ^ 1) * UF2_STAGE;
            const bool last = kc + 1 == kchunks;
            const bool issue = !last || have_next;
            uint32_t kcn;
            if (!last) { kcn = kr; kr = kr + 1 == kchunks ? 0 : kr + 1; }
            else kcn = krn;
            load_w(so, 0, 1, w1);
            UF2_LGKM_WAIT(4);  // a0, w0 are back
            mfma16(a0, w0, 0, issue, last, 0, kcn, nbuf);
            load_a(so, 1, a1);
            load_w(so, 1, 0, w0);
            UF2_LGKM_WAIT(8);  // w1
            mfma16(a0, w1, 4, issue, last, 4, kcn, nbuf);
            load_w(so, 1, 1, w1);
            UF2_LGKM_WAIT(4);  // a1, w0
            mfma16(a1, w0, 0, false, false, 0, 0, nbuf);
            UF2_LGKM_WAIT(0);  // w1: this wave's last reads of the stage are back
            if (!last) {
                sh_wait_vmcnt<0>();  // its pieces of the next stage have landed
                __builtin_amdgcn_s_barrier();
                __builtin_amdgcn_sched_barrier(0);
                load_a(so ^ UF2_STAGE, 0, a0);
                load_w(so ^ UF2_STAGE, 0, 0, w0);
                __builtin_amdgcn_sched_barrier(0);
            }
            mfma16(a1, w1, 4, false, false, 0, 0, nbuf);
        }
        // threshold epilogue of (mt, nt) while the next tile's stage 0 is in flight
        // (C/D of the 16x16 MFMA: query = lane & 15, row = 4 (lane >> 4) + r)
        const uint32_t m0 = mt * UF2_BM, n0 = nt * UF2_BN;
        float4 tmv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if constexpr (I8) tmv = tmeta[(row_lo >> 7) + 2 * mt + (wr >> 1)];  // uniform: a scalar load (rows past M: masked)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t q = n0 + wc * 128 + j * 16 + l15;
            const bool qok = q < nq;
            // f16: score > tau - margin.  int8: I > floor((tau - slack) inv_q inv_t - 0.5001 (A_q + B_t) - ...), as an
            // integer compare; a NaN threshold (flagged tile) or tau = -inf takes every row
            float tq = 0.0f;
            int ti = 0;
            bool all = false;
            if constexpr (I8) {
                const float4 qm = qmeta[qok ? q : 0];
                const float T = q8_threshold((tau[qok ? q : 0] - margin - qm.z) * qm.x, qm.y, qm.w, qmeta[nq + (qok ? q : 0)].x, tmv,
                                             kQ8Quarter * 128.0f * (float)kchunks);
                all = !(T == T) || T < -2.0e9f;
                ti = T > 2.0e9f ? 0x7fffffff : (int)T;
            } else {
                tq = qok ? tau[q] - margin : 0.0f;
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t m = m0 + wr * 64 + i * 16 + 4 * g + r;
                    bool hit;
                    if constexpr (I8) hit = all || acc[i][j][r] > ti;
                    else hit = !(acc[i][j][r] <= tq);
                    if (qok && m < M && hit) {
                        const uint64_t row = row_lo + m;
                        if (!dead || !((dead[row >> 5] >> (row & 31)) & 1u)) {
                            const uint32_t pos = atomicAdd(&cnt[(size_t)q * kCntStride], 1u);
                            if (pos < cap) cand[2 * ((size_t)q * cap + pos)] = (uint32_t)row;  // low word of the 8-byte slot
                        }
                    }
                }
            }
        }
        if (!have_next) break;
        par = (par + kchunks) & 1;
        slot = slot_n;
        mt = mtn;
        nt = ntn;
#pragma unroll
        for (int i = 0; i < 4; ++i) { a_cur[i] = a_nxt[i]; w_cur[i] = w_nxt[i]; }
        kr = krn + 1 == kchunks ? 0 : krn + 1;  // stage 0 (chunk krn) is already on its way
    }
#undef UF2_LGKM_WAIT
}

// ---- up to 64 queries: resident queries, deep corpus ring ---------------------------------------
// With few queries the filter is a pure stream of the f16 corpus copy, and what limits a
// tile-at-a-time kernel is bytes in flight per CU (one 16 KB corpus stage per block) against HBM
// latency.  Here one persistent block per CU keeps its 32*NQT unit queries in LDS for its whole
// life and gives the corpus a ring in the remaining LDS: each of the 4 waves owns 32 rows of a 128-row
// tile and a private ring of R 4-KiB slots filled by LDS-DMA, R-1 stages (3 x 16 KB per CU at
// NQT = 1, see RCAP) in flight across tile boundaries under counted vmcnt — no barrier in the loop,
// since a wave only reads rows it loaded itself.
template <int NQT, int KC = 6, int RCAP_ = (NQT == 1 ? 4 : 8)>  // KC = dim / 64 k-chunks per row: 6 / 12 / 16 for dim 384 / 768 / 1024
struct RwGeom {
    static constexpr int QROWS = 32 * NQT;
    static constexpr int WBYTES = KC * QROWS * 128;            // resident queries: KC chunks x QROWS x 128 B
    static constexpr int PEND = (int)kPend;                    // pending candidates per wave (8 B each)
    static constexpr int RMAX = (160 * 1024 - 4 * PEND * 8 - WBYTES) / 16384;
    // Up to 32 queries the ring stops at 4 slots (3 stages = 48 KiB in flight per CU) although LDS would hold 8:
    // the memory system rewards fewer outstanding requests (benchmarks/hbm_read_probe.hip; 8 queries over
    // 10M x 384: 1.284 -> 1.270 ms, 9 queries k = 200: 1.420 -> 1.413; 3 slots measure the same, 768 / 1024-d
    // within 0.5 % either way).
    static constexpr int RCAP = RCAP_;
    static constexpr int R = RMAX > RCAP ? RCAP : RMAX;              // ring slots (16 KiB each, 4 KiB per wave):
                                                               // dim 384: 4 / 6 / 3 at NQT 1 / 2 / 4; 768: 4 / 3; 1024: 4
    static constexpr int LDS = WBYTES + R * 16384;             // dim 384: 90,112 / 147,456 / 147,456 B
    static constexpr int LDS_ALL = LDS + 4 * PEND * 8;         // + 4 KiB
    static_assert(R >= 3, "the ring needs at least two stages in flight");
};

template <int N>
__device__ __forceinline__ void uf_wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int NQT, int KC>
__global__ void __launch_bounds__(256)
score_filter_rw_kernel(const _Float16* __restrict__ corpus_h, uint64_t row_lo, uint64_t row_hi,
                       const _Float16* __restrict__ queries_h, uint32_t nq, const float* __restrict__ tau,
                       const uint32_t* __restrict__ dead, uint32_t* __restrict__ cand,
                       uint32_t* __restrict__ cnt, uint32_t cap, uint32_t qtiles, uint32_t nt_stream, float margin) {
    using G = RwGeom<NQT, KC>;
    // one query tile: every corpus byte is read by exactly one CU, once — stream it past the caches (with
    // several query tiles the blocks of an XCD share tiles through its L2: default policy)
    const bool NT = nt_stream != 0 && qtiles == 1;
    constexpr int R = G::R;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* Wl = lds;                 // [KC][QROWS][128 B], slots swizzled as in uf_mainloop
    char* ring = lds + G::WBYTES;   // [R][4 waves][32 rows][128 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const uint64_t M = row_hi - row_lo;
    const uint64_t ntile = (M + 127) / 128;
    const _Float16* base = corpus_h + uf_tiled_off(row_lo, 0, KC);  // row_lo is a multiple of 128
    // Several query tiles: blocks of one XCD (blockIdx % 8) that hold different query tiles share a
    // row group and walk its corpus tiles in the same order, so a tile comes from HBM once per XCD
    // group and from that XCD's L2 for the other query tiles.
    const uint32_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const uint32_t qt = slot % qtiles, rg = slot / qtiles, rgn = (gridDim.x >> 3) / qtiles;
    if (rg >= rgn) return;  // spare slot when qtiles does not divide the slots of an XCD
    const uint32_t q0 = qt * G::QROWS;

    // resident queries: 8 rows x 128 B per instruction, KC*NQT instructions per wave
#pragma unroll
    for (int i = 0; i < KC * NQT; ++i) {
        const int g8 = wave * KC * NQT + i;              // group of 8 (chunk, row) lines
        const int c = g8 / (4 * NQT), r8 = g8 % (4 * NQT);
        const int row = r8 * 8 + (lane >> 3);
        const int pc = (lane & 7) ^ ((row >> 1) & 7);
        const uint32_t q = q0 + row < nq ? q0 + row : nq - 1;
        sh_glds16(queries_h + (size_t)q * (KC * 64) + c * 64 + pc * 8, Wl + (c * G::QROWS + r8 * 8) * 128);
    }
    uf_wait_vmcnt<0>();
    __syncthreads();

    float tq[NQT];
    bool qok[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = q0 + 32 * t + l31;
        qok[t] = q < nq;
        tq[t] = qok[t] ? tau[q] - margin : 0.0f;
    }

    // this wave's staging: 4 instructions of 8 rows per stage; lane -> (row 8i + lane/8, slot lane%8)
    const int swz = (l31 >> 1) & 7;
    int a_sl[4], w_off[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) {
        a_sl[st] = l31 * 128 + (((2 * st + h) ^ swz) * 16);
        w_off[st] = l31 * 128 + (((2 * st + h) ^ swz) * 16);
    }
    char* myring = ring + wave * 4096;
    auto issue = [&](uint64_t tile, int c, int slot) {  // stage (tile, chunk c) -> ring slot
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i * 8 + (lane >> 3);
            const int pc = (lane & 7) ^ ((row >> 1) & 7);
            // 8 consecutive rows of chunk c = 1 KiB of consecutive lines (rows past M: padded tile, masked at append)
            if (NT) sh_glds16_nt(base + ((tile * KC + c) * 128 + wave * 32 + row) * 64 + pc * 8, myring + slot * 16384 + i * 1024);
            else sh_glds16(base + ((tile * KC + c) * 128 + wave * 32 + row) * 64 + pc * 8, myring + slot * 16384 + i * 1024);
        }
    };

    const uint64_t t0 = (uint64_t)rg * 8 + xcd, tstep = (uint64_t)rgn * 8;
    if (t0 >= ntile) return;
    // flattened stage sequence g = n*KC + c over this block's tiles; ring slot = g % R
    const uint64_t my_tiles = (ntile - t0 + tstep - 1) / tstep;
    const uint64_t nstage = my_tiles * KC;
    uint64_t gi = 0;              // next stage to issue = (tile i_tile, chunk i_c) -> slot i_slot
    uint64_t i_tile = t0;
    int i_c = 0, i_slot = 0;
    auto issue_next = [&]() {
        issue(i_tile, i_c, i_slot);
        ++gi;
        if (++i_c == KC) { i_c = 0; i_tile += tstep; }
        if (++i_slot == R) i_slot = 0;
    };
    for (int p = 0; p < R - 1; ++p)
        if (gi < nstage) issue_next();

    // this wave's pending candidates (cand_push / cand_flush)
    volatile uint64_t* pend = reinterpret_cast<volatile uint64_t*>(lds + G::LDS) + wave * kPend;
    uint32_t npend = 0;  // wave-uniform

    sh_f32x16 acc[NQT];
    int c_slot = 0;  // ring slot of the stage being consumed
    for (uint64_t n = 0; n < my_tiles; ++n) {
        const uint64_t tile = t0 + n * tstep;
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            // the slot refilled now was read in the previous iteration: its ds_reads are back
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (gi < nstage) {
                issue_next();
                uf_wait_vmcnt<4 * (R - 1)>();  // all but the R-1 youngest stages have landed: stage g is in
            } else {
                uf_wait_vmcnt<0>();            // tail: nothing younger to keep in flight
            }
            const char* slot = myring + c_slot * 16384;
            if (++c_slot == R) c_slot = 0;
            const char* wc = Wl + c * G::QROWS * 128;
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const f16x8 a = *reinterpret_cast<const f16x8*>(slot + a_sl[st]);
#pragma unroll
                for (int t = 0; t < NQT; ++t) {
                    const f16x8 w = *reinterpret_cast<const f16x8*>(wc + t * 32 * 128 + w_off[st]);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, w, acc[t], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint64_t m = tile * 128 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                cand_push(qok[t] && m < M && !(acc[t][r] <= tq[t]), q0 + 32 * t + l31, row_lo + m, dead, pend, npend,
                          lane, cand, cnt, cap);
            }
        }
    }
    cand_flush(pend, npend, lane, cand, cnt, cap);
}

// Refine, step 1: exact cosines of the candidates, in place.  A candidate is an 8-byte slot of
// cand[q][cap] whose low word the filter set to the row number; this kernel overwrites the slot
// with the packed (cosine, id) key (0 for a NaN/Inf score), one half-wave per row with the layout
// and operation order of scan_topk_kernel.  Step 2 is select_candidates_kernel (scan_mfma.hip).
// The rows of ONE query are spread over gridDim.x blocks: a CU pulls ~50 GB/s of scattered 1.5-KB
// rows, so the ~500 candidates a k = 200 phase brings per query took 32 us on one CU (9 queries:
// 9 CUs busy, 247 idle) and take ~3 us on 32.
constexpr int RK_THREADS = 256;
// LIST (phase 0 of a scoped search, scoped_filter_plan.hpp; first_rows != 0): candidate i is row dead[i] — the scope's
// ascending row list is passed where the tombstone bitmap goes, and it holds live rows only, so no bit is tested.
template <int J, bool LIST = false>
__global__ void __launch_bounds__(RK_THREADS)
rescore_keys_kernel(const float* __restrict__ corpus, const float* __restrict__ queries,
                    const float* __restrict__ qmag, uint64_t* __restrict__ cand,
                    const uint32_t* __restrict__ cnt, uint32_t cap, RowIds id_base,
                    uint32_t first_rows, const uint32_t* __restrict__ dead) {
    constexpr int DIM = 128 * J;
    constexpr int RU = J <= 3 ? 4 : 2;          // rows per half-wave per round, loads issued together
    constexpr int PER = RU * (RK_THREADS / 32);  // candidates per block per round
    const int tid = threadIdx.x, l32 = tid & 31;
    const uint32_t hw = tid >> 5;
    const uint32_t q = blockIdx.y;
    // first_rows != 0: phase 0 — candidate i IS row i (tau is still -inf, the filter would append
    // every row: a million atomics at 1,000 queries); tombstoned rows become empty keys
    uint32_t n = first_rows ? first_rows : cnt[(size_t)q * kCntStride];
    if (n > cap) n = cap;  // select_candidates_kernel raises the overflow flag
    if (blockIdx.x * PER >= n) return;
    f32x4 qf[J];
    {
        const f32x4* qp = reinterpret_cast<const f32x4*>(queries + (size_t)q * DIM) + l32;
#pragma unroll
        for (int j = 0; j < J; ++j) qf[j] = qp[j * 32];
    }
    const float qm = qmag[q];
    uint64_t* slots = cand + (size_t)q * cap;
    for (uint32_t i0 = blockIdx.x * PER; i0 < n; i0 += gridDim.x * PER) {
        f32x4 v[RU][J];
        uint32_t row[RU];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (RK_THREADS / 32) + hw;  // half-wave uniform
            row[u] = (i < n) ? (first_rows ? (LIST ? dead[i] : i) : (uint32_t)slots[i]) : 0u;
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (RK_THREADS / 32) + hw;
            if (i < n) {
                const f32x4* p = reinterpret_cast<const f32x4*>(corpus + (size_t)row[u] * DIM) + l32;
#pragma unroll
                for (int j = 0; j < J; ++j) v[u][j] = p[j * 32];
            }
        }
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (RK_THREADS / 32) + hw;
            if (i < n) {  // xor masks <= 16 stay inside the half-wave
                float ss = 0.0f, dot = 0.0f;
#pragma unroll
                for (int j = 0; j < J; ++j) {
                    ss = fmaf(v[u][j].x, v[u][j].x, ss); ss = fmaf(v[u][j].y, v[u][j].y, ss);
                    ss = fmaf(v[u][j].z, v[u][j].z, ss); ss = fmaf(v[u][j].w, v[u][j].w, ss);
                    dot = fmaf(v[u][j].x, qf[j].x, dot); dot = fmaf(v[u][j].y, qf[j].y, dot);
                    dot = fmaf(v[u][j].z, qf[j].z, dot); dot = fmaf(v[u][j].w, qf[j].w, dot);
                }
                const float xmag = sqrtf(half_sum_s(ss));
                const float d = half_sum_s(dot);
                const float c = (qm == 0.0f || xmag == 0.0f) ? 0.0f : d / (qm * xmag);  // batch.rs:320-323
                // NaN/Inf scores are never returned
                const bool live = LIST || !(first_rows && dead) || !((dead[row[u] >> 5] >> (row[u] & 31)) & 1u);
                if (l32 == 0)
                    slots[i] = (live && c > -__builtin_huge_valf() && c < __builtin_huge_valf()) ? key_pack(c, id_base.of(row[u])) : 0ull;
            }
        }
    }
}

// ---- int8 filter copy -----------------------------------------------------------------------------
// A third, quarter-size copy of the corpus for the resident-query kernel: unit rows quantised to int8 with one
// scale per 128-row tile, scored on v_mfma_i32_32x32x32_i8 (exact integer dot products), the same 16-KiB stages,
// LDS image and ring as score_filter_rw_kernel — a 128-B line now holds 128 k instead of 64, so a 384-d tile
// is 3 stages instead of 6 and the filter streams 1 byte per element.
//
//   u_i = x_i / |x|  (f32, the arithmetic of unit_f16_rows_kernel);  inv_t = 127 / max |u_i| over the tile;
//   a_i = rint(u_i * inv_t)  in [-127, 127];   queries the same with their own inv_q, b_i = rint(v_i * inv_q).
//
// Bound.  With s_t = 1 / inv_t, s_q = 1 / inv_q:  u_i = s_t (a_i + e_i),  v_i = s_q (b_i + d_i),  |e_i|, |d_i| <=
// 0.5 + 127 * 2^-24 (the f32 rounding of the product before rint), so
//   sum u_i v_i = s_t s_q (I + sum b_i e_i + sum a_i d_i + sum e_i d_i),   I = sum a_i b_i  (the MFMA's output, exact)
//   |sum u_i v_i - s_t s_q I| <= s_t s_q (0.5001 (A_q + B_t) + 0.2501 dim),   A_q = sum |b_i|,  B_t = max over the tile's rows of sum |a_i|.
// Each of the three error sums is also bounded by Cauchy-Schwarz — |sum b_i e_i| <= |b| |e| with the rows' ACTUAL
// error norms, which the quantiser measures (sqrt(dim / 12) per unit of scale for evenly spread values, against the
// worst case 0.5 sqrt(dim)) — and the kernels take whichever side is smaller per (tile, query) (q8_threshold): the
// L1 side for sparse or one-hot vectors, the Cauchy-Schwarz side (~0.7 of it) for evenly spread ones.
// The refine's cosine differs from sum u_i v_i by f32 rounding only (<= dim * 2^-23 + 4e-5, kQ8Slack).  A row whose
// exact cosine beats tau therefore has
//   I > (tau - slack) * inv_q * inv_t - min(0.5001 A_q, |b| E_t) - min(0.5001 B_t, N_t |d|) - min(0.2501 dim, E_t |d|)
// and the kernel appends every row above that line lowered by 4 more units (rounding of the f32 expression itself:
// its terms stay below 2^23, inv <= 127 sqrt(dim)).  In cosine units the band is ~0.017 at 384-d for Gaussian-like
// rows (0.024 on the L1 side alone; the f16 copy: 0.001): a few dozen extra candidates per query at k = 10 over 10M
// random rows, a couple of thousand per phase at k = 200 — against half the bytes streamed.  A tile holding a non-finite value has inv_t = NaN and all its
// rows become candidates (the refine decides).  Only complete tiles are quantised (a tile is written once, when
// cs_index_build first sees it full: a search running beside a build never reads a tile being rewritten); the rows
// behind the last complete tile are appended as candidates outright (tail_candidates_kernel, < 128 rows).
// mu[c] = mean over rows [0, n) of x[c] / |x| (rows of zero or non-finite norm count as zero rows): column sums per
// block in registers (thread t owns columns t, t + 256, ...: a row is read coalesced), one atomicAdd per column per
// block into `sum`; mean_finish_kernel divides.  Summation order varies run to run: mu only has to be the SAME vector
// for the quantiser and the queries, any vector keeps the filter exact.
__global__ void __launch_bounds__(256)
unit_mean_kernel(const float* __restrict__ corpus, const float* __restrict__ row_norm, uint64_t n, uint32_t dim,
                 float* __restrict__ sum) {
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // dim <= 1024
    for (uint64_t r = blockIdx.x; r < n; r += gridDim.x) {
        const float nrm = row_norm[r];
        if (!(nrm > 0.0f && nrm < __builtin_huge_valf())) continue;
        const float inv = 1.0f / nrm;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = threadIdx.x + 256 * i;
            if (c < dim) {
                const float u = corpus[r * dim + c] * inv;
                if (u == u) acc[i] += u;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t c = threadIdx.x + 256 * i;
        if (c < dim) atomicAdd(&sum[c], acc[i]);
    }
}
__global__ void mean_finish_kernel(float* __restrict__ mu, uint32_t dim, float inv_n) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c < dim) {
        const float m = mu[c] * inv_n;
        mu[c] = (m == m && fabsf(m) <= 1.0f) ? m : 0.0f;
    }
}

// One block per 128-row tile (tiles tile0 .. tile0 + gridDim.x - 1): pass 1 finds the tile's largest unit magnitude,
// pass 2 (the tile is in L2 now) quantises.  A half-wave per row; lane l32 holds float4 l32 + 32 j of the row, i.e.
// bytes 4 l32 .. 4 l32 + 3 of the row's line in k-chunk j of [tile][chunk of 128 k][row][128 B].
template <int J>
__global__ void __launch_bounds__(256)
corpus_q8_kernel(const float* __restrict__ corpus, const float* __restrict__ row_norm, int8_t* __restrict__ q8,
                 float4* __restrict__ tmeta, uint64_t tile0, const float* __restrict__ mu) {
    constexpr int DIM = 128 * J;
    __shared__ float s_max[8], s_err[8], s_sq[8];
    __shared__ int s_bad[8], s_abs[8];
    const uint64_t tile = tile0 + blockIdx.x;
    const int tid = threadIdx.x, l32 = tid & 31, hw = tid >> 5;
    f32x4 mv[J];
#pragma unroll
    for (int j = 0; j < J; ++j) mv[j] = *reinterpret_cast<const f32x4*>(mu + (l32 + 32 * j) * 4);
    float mx = 0.0f;
    int bad = 0;
    for (int r = hw; r < 128; r += 8) {
        const uint64_t row = tile * 128 + r;
        const float nrm = row_norm[row];
        const f32x4* p = reinterpret_cast<const f32x4*>(corpus + row * DIM) + l32;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const f32x4 v = p[j * 32];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float u = fabsf((nrm == 0.0f ? 0.0f : v[e] / nrm) - mv[j][e]);
                if (!(u < __builtin_huge_valf())) bad = 1;
                mx = fmaxf(mx, u);
            }
        }
    }
    mx = half_max_q8(mx);
    bad = half_sum_i(bad);
    if (l32 == 0) { s_max[hw] = mx; s_bad[hw] = bad; }
    __syncthreads();
    mx = 0.0f;
    bad = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { mx = fmaxf(mx, s_max[i]); bad |= s_bad[i]; }
    const float inv = mx > 0.0f ? 127.0f / mx : 1.0f;
    int bmax = 0;
    float emax = 0.0f, smax = 0.0f;  // largest squared error norm / squared norm of a row
    for (int r = hw; r < 128; r += 8) {
        const uint64_t row = tile * 128 + r;
        const float nrm = row_norm[row];
        const f32x4* p = reinterpret_cast<const f32x4*>(corpus + row * DIM) + l32;
        int abs_sum = 0;
        float sq_sum = 0.0f, err_sum = 0.0f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const f32x4 v = p[j * 32];
            f32x4 u;
#pragma unroll
            for (int e = 0; e < 4; ++e) u[e] = (nrm == 0.0f ? 0.0f : v[e] / nrm) - mv[j][e];
            const uint32_t w = q8_pack4(u, inv, abs_sum, sq_sum, err_sum);
            *reinterpret_cast<uint32_t*>(q8 + ((tile * J + j) * 128 + r) * 128 + l32 * 4) = w;
        }
        abs_sum = half_sum_i(abs_sum);
        bmax = abs_sum > bmax ? abs_sum : bmax;
        emax = fmaxf(emax, half_sum_s(err_sum));
        smax = fmaxf(smax, half_sum_s(sq_sum));
    }
    if (l32 == 0) { s_abs[hw] = bmax; s_err[hw] = emax; s_sq[hw] = smax; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            bmax = s_abs[i] > bmax ? s_abs[i] : bmax;
            emax = fmaxf(emax, s_err[i]);
            smax = fmaxf(smax, s_sq[i]);
        }
        tmeta[tile] = make_float4(bad ? __builtin_nanf("") : inv, kQ8Half * (float)bmax, sqrtf(emax) * 1.001f + 1.0e-3f,
                                  sqrtf(smax) * 1.0001f);
    }
}

// rows [lo, hi) (fewer than 128: the incomplete last tile) become candidates of every query
__global__ void __launch_bounds__(128)
tail_candidates_kernel(uint64_t lo, uint64_t hi, const uint32_t* __restrict__ dead, uint32_t* __restrict__ cand,
                       uint32_t* __restrict__ cnt, uint32_t cap) {
    const uint32_t q = blockIdx.x;
    const uint64_t row = lo + threadIdx.x;
    if (row >= hi) return;
    if (dead && ((dead[row >> 5] >> (row & 31)) & 1u)) return;
    const uint32_t pos = atomicAdd(&cnt[(size_t)q * kCntStride], 1u);
    if (pos < cap) cand[2 * ((size_t)q * cap + pos)] = (uint32_t)row;
}

// Ring depth of the int8 kernel (slots of 16 KiB; R - 1 stages in flight per CU).  Up to 32 queries: 3 — 8 queries
// k = 10 over 10M x 384: 0.687 ms at 3, 0.704 at 4, 0.698 / 0.704 at 6 / 8 (the f16 kernel's finding, one step further).
#ifndef CS_RW8_RCAP1
#define CS_RW8_RCAP1 3
#endif
#ifndef CS_RW8_RCAP2
#define CS_RW8_RCAP2 8
#endif
template <int NQT, int KC>
using Rw8Geom = RwGeom<NQT, KC, (NQT == 1 ? CS_RW8_RCAP1 : CS_RW8_RCAP2)>;

// score_filter_rw_kernel over the int8 copy.  KC = dim / 128 stages per tile; rows [row_lo, row_hi) are whole tiles.
// TWO: the queries in two int8 planes (prep_queries_kernel: 128 hi + lo, a 128 times finer query scale) — a second
// query image in LDS and a second MFMA per step into a second accumulator set, combined as 128 I_hi + I_lo in the
// epilogue; queries_q8 is the hi plane, queries_lo the lo plane, and the query constants are the finer unit's.
template <int NQT, int KC, bool TWO>
using Rw8GeomT = typename std::conditional<TWO, RwGeom<2 * NQT, KC, (NQT == 1 ? CS_RW8_RCAP1 : CS_RW8_RCAP2)>, Rw8Geom<NQT, KC>>::type;

template <int NQT, int KC, bool TWO = false>
__global__ void __launch_bounds__(256)
score_filter_rw8_kernel(const int8_t* __restrict__ corpus_q8, const float4* __restrict__ tmeta, uint64_t row_lo,
                        uint64_t row_hi, const int8_t* __restrict__ queries_q8, const float4* __restrict__ qmeta,
                        uint32_t nq, const float* __restrict__ tau, const uint32_t* __restrict__ dead,
                        uint32_t* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap, uint32_t qtiles,
                        uint32_t nt_stream, float slack, const int8_t* __restrict__ queries_lo = nullptr) {
    using G = Rw8GeomT<NQT, KC, TWO>;
    constexpr int QROWS = 32 * NQT;              // (G::QROWS counts both planes when TWO)
    constexpr int WB1 = KC * QROWS * 128;        // one plane of the query image
    const bool NT = nt_stream != 0 && qtiles == 1;
    constexpr int R = G::R;
    constexpr int DIM = 128 * KC;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* Wl = lds;                 // [KC][QROWS][128 B], slots swizzled as in uf_mainloop (TWO: the lo plane behind it)
    char* ring = lds + G::WBYTES;   // [R][4 waves][32 rows][128 B]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, h = lane >> 5;
    const uint64_t tile_lo = row_lo >> 7;  // row_lo, row_hi are multiples of 128
    const uint64_t ntile = (row_hi - row_lo) >> 7;
    const int8_t* base = corpus_q8 + tile_lo * KC * 128 * 128;
    const float4* tm = tmeta + tile_lo;
    const uint32_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const uint32_t qt = slot % qtiles, rg = slot / qtiles, rgn = (gridDim.x >> 3) / qtiles;
    if (rg >= rgn) return;
    const uint32_t q0 = qt * QROWS;

#pragma unroll
    for (int i = 0; i < KC * NQT; ++i) {
        const int g8 = wave * KC * NQT + i;
        const int c = g8 / (4 * NQT), r8 = g8 % (4 * NQT);
        const int row = r8 * 8 + (lane >> 3);
        const int pc = (lane & 7) ^ ((row >> 1) & 7);
        const uint32_t q = q0 + row < nq ? q0 + row : nq - 1;
        sh_glds16(reinterpret_cast<const _Float16*>(queries_q8 + (size_t)q * DIM + c * 128 + pc * 16),
                  Wl + (c * QROWS + r8 * 8) * 128);
        if (TWO)
            sh_glds16(reinterpret_cast<const _Float16*>(queries_lo + (size_t)q * DIM + c * 128 + pc * 16),
                      Wl + WB1 + (c * QROWS + r8 * 8) * 128);
    }
    uf_wait_vmcnt<0>();
    __syncthreads();

    // per query (lane & 31): tqs = (tau - slack - q.mu) * inv_q and the three constants of q8_threshold
    float tqs[NQT], hA[NQT], nb[NQT], Dq[NQT];
    bool qok[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) {
        const uint32_t q = q0 + 32 * t + l31;
        qok[t] = q < nq;
        const float4 m = qmeta[(TWO ? 2 * nq : 0) + (qok[t] ? q : 0)];
        tqs[t] = (tau[qok[t] ? q : 0] - slack - m.z) * m.x;
        hA[t] = m.y;
        nb[t] = m.w;
        Dq[t] = qmeta[(TWO ? 3 * nq : nq) + (qok[t] ? q : 0)].x;
    }

    const int swz = (l31 >> 1) & 7;
    int a_sl[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) a_sl[st] = l31 * 128 + (((2 * st + h) ^ swz) * 16);
    char* myring = ring + wave * 4096;
    auto issue = [&](uint64_t tile, int c, int slot) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = i * 8 + (lane >> 3);
            const int pc = (lane & 7) ^ ((row >> 1) & 7);
            const _Float16* src = reinterpret_cast<const _Float16*>(base + ((tile * KC + c) * 128 + wave * 32 + row) * 128 + pc * 16);
            if (NT) sh_glds16_nt(src, myring + slot * 16384 + i * 1024);
            else sh_glds16(src, myring + slot * 16384 + i * 1024);
        }
    };

    const uint64_t t0 = (uint64_t)rg * 8 + xcd, tstep = (uint64_t)rgn * 8;
    if (t0 >= ntile) return;
    const uint64_t my_tiles = (ntile - t0 + tstep - 1) / tstep;
    const uint64_t nstage = my_tiles * KC;
    uint64_t gi = 0;
    uint64_t i_tile = t0;
    int i_c = 0, i_slot = 0;
    auto issue_next = [&]() {
        issue(i_tile, i_c, i_slot);
        ++gi;
        if (++i_c == KC) { i_c = 0; i_tile += tstep; }
        if (++i_slot == R) i_slot = 0;
    };
    for (int p = 0; p < R - 1; ++p)
        if (gi < nstage) issue_next();

    volatile uint64_t* pend = reinterpret_cast<volatile uint64_t*>(lds + G::LDS) + wave * kPend;
    uint32_t npend = 0;  // wave-uniform

    i32x16 acc[NQT], acc_lo[TWO ? NQT : 1];
    int c_slot = 0;
    // tile scales: scalar loads (uniform address, read-only data) — they count on lgkmcnt, not on the vmcnt the ring
    // is paced by — fetched one tile ahead
    float4 tm_next = tm[t0];
    for (uint64_t n = 0; n < my_tiles; ++n) {
        const uint64_t tile = t0 + n * tstep;
        const float4 tmv = tm_next;
        tm_next = tm[n + 1 < my_tiles ? tile + tstep : tile];
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[t][r] = 0;
                if (TWO) acc_lo[t][r] = 0;
            }
#pragma unroll
        for (int c = 0; c < KC; ++c) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (gi < nstage) {
                issue_next();
                uf_wait_vmcnt<4 * (R - 1)>();
            } else {
                uf_wait_vmcnt<0>();
            }
            const char* slot = myring + c_slot * 16384;
            if (++c_slot == R) c_slot = 0;
            const char* wc = Wl + c * QROWS * 128;
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                const i32x4 a = *reinterpret_cast<const i32x4*>(slot + a_sl[st]);
#pragma unroll
                for (int t = 0; t < NQT; ++t) {
                    const i32x4 w = *reinterpret_cast<const i32x4*>(wc + t * 32 * 128 + a_sl[st]);
                    acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, w, acc[t], 0, 0, 0);
                    if (TWO) {
                        const i32x4 wl = *reinterpret_cast<const i32x4*>(wc + WB1 + t * 32 * 128 + a_sl[st]);
                        acc_lo[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, wl, acc_lo[t], 0, 0, 0);
                    }
                }
            }
        }
#pragma unroll
        for (int t = 0; t < NQT; ++t) {
            // I > T  <=>  I > floor(T) for an integer I; NaN (flagged tile or query) -> every row
            const float T = q8_threshold(tqs[t], hA[t], nb[t], Dq[t], tmv, kQ8Quarter * (float)DIM);
            const int Ti = (T == T) ? (T < -2.0e9f ? (int)0x80000000 : (T > 2.0e9f ? 0x7fffffff : (int)T)) : (int)0x80000000;
            const bool all = !(T == T) || T < -2.0e9f;
            if (TWO) {  // I = 128 I_hi + I_lo (|I| <= 127 * 16,256 * dim < 2^31 up to dim 768)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[t][r] = acc[t][r] * 128 + acc_lo[t][r];
            }
            // most tiles hold no candidate for anybody: one test of the lane's largest product instead of sixteen
            int top = acc[t][0];
#pragma unroll
            for (int r = 1; r < 16; ++r) top = acc[t][r] > top ? acc[t][r] : top;
            if (!__ballot(qok[t] && (all || top > Ti))) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint64_t m = tile * 128 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                cand_push(qok[t] && (all || acc[t][r] > Ti), q0 + 32 * t + l31, row_lo + m, dead, pend, npend, lane, cand,
                          cnt, cap);
            }
        }
    }
    cand_flush(pend, npend, lane, cand, cnt, cap);
}

// ---- many queries over the int8 copy: two waves per SIMD ---------------------------------------------
// With 256 resident queries score_filter_rw8_kernel<8, 3> runs ONE wave per SIMD (its ring and the query image fill
// the LDS, its accumulators half the registers), and a wave issues in order: the 1-KiB LDS read behind every MFMA, the
// MFMAs and the threshold epilogue add up instead of overlapping (ablations in DESIGN.md 9.0c: ~2 us of LDS reads + ~2
// us of MFMAs + 0.9 us of epilogue per 128 rows x 256 queries).  Here a block is EIGHT waves — two per SIMD, 256
// registers each: 128 accumulators + at most 128 others — over one query image: a wave's corpus fragments never
// touch LDS (lane (row l31, half h) loads its 16 B of MFMA step st — bytes (2 st + h) * 16 of the row's 128-B line, the
// k order of the query image — with plain global loads, one unit ahead), so LDS holds only the queries and while one
// wave of a SIMD waits for its query fragments or works through an epilogue the other one feeds the matrix pipe.
// A unit is 256 rows (two corpus tiles): wave w owns rows 32 w .. 32 w + 31 of it.  1,000 queries over 10M rows:
// 5.9 -> 4.8 ms per search (512: 3.2 -> 2.5; 129: 1.6 -> 1.45).  Ablations of the last phase (3.81 ms): 3.08 without
// the epilogue, 1.68 with one MFMA in eight — the MFMAs' share (4.2 us per unit) is close to what the matrix pipe
// sustains on such operands (3.8), and what is left (LDS reads, epilogue, loads: 3.3 us) still adds to it rather
// than hiding under it: the part is power-limited, and time follows the energy of everything a kernel does.
template <int I, int N, typename F>
__device__ __forceinline__ void cs_static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        cs_static_for<I + 1, N>(f);
    }
}

template <int NQT, int KC>
constexpr int kRq8Lds = KC * 32 * NQT * 128 + 8 * (int)kPend * 8 + 32 * NQT * 16;  // the query image + eight pending-candidate
                                                                                   // lists + the queries' threshold constants

template <int NQT, int KC, bool NT>
__global__ void __launch_bounds__(512)
score_filter_rq8_kernel(const int8_t* __restrict__ corpus_q8, const float4* __restrict__ tmeta, uint64_t row_lo,
                        uint64_t row_hi, const int8_t* __restrict__ queries_q8, const float4* __restrict__ qmeta,
                        uint32_t nq, const float* __restrict__ tau, const uint32_t* __restrict__ dead,
                        uint32_t* __restrict__ cand, uint32_t* __restrict__ cnt, uint32_t cap, uint32_t qtiles,
                        float slack) {
    constexpr int DIM = 128 * KC;
    constexpr int QROWS = 32 * NQT;
    constexpr int WBYTES = KC * QROWS * 128;
    extern __shared__ __attribute__((aligned(16))) char lds[];
    char* Wl = lds;  // [KC][QROWS][128 B], slots swizzled as in uf_mainloop
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // 0 .. 7
    const int l31 = lane & 31, h = lane >> 5;
    const uint64_t M = row_hi - row_lo;            // a multiple of 128 (whole corpus tiles)
    const uint64_t nunit = (M + 255) / 256;        // the last unit may hold one real tile: its second tile is
                                                   // allocated (even tile count) and its rows are masked
    const uint64_t tile_lo = row_lo >> 7;
    const uint32_t xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const uint32_t qt = slot % qtiles, rg = slot / qtiles, rgn = (gridDim.x >> 3) / qtiles;
    if (rg >= rgn) return;
    const uint32_t q0 = qt * QROWS;

    // resident queries: 8 rows x 128 B per instruction, KC * NQT * 4 instructions over eight waves
    for (int g8 = wave; g8 < KC * NQT * 4; g8 += 8) {
        const int c = g8 / (4 * NQT), r8 = g8 % (4 * NQT);
        const int row = r8 * 8 + (lane >> 3);
        const int pc = (lane & 7) ^ ((row >> 1) & 7);
        const uint32_t q = q0 + row < nq ? q0 + row : nq - 1;
        sh_glds16(queries_q8 + (size_t)q * DIM + c * 128 + pc * 16, Wl + (c * QROWS + r8 * 8) * 128);
    }
    uf_wait_vmcnt<0>();
    __syncthreads();

    // per resident query {tqs, hA, nb, Dq} (q8_threshold) in LDS: four registers per query tile would cost the
    // second wave per SIMD
    float4* qv = reinterpret_cast<float4*>(lds + WBYTES + 8 * kPend * 8);  // [QROWS]
    bool qok[NQT];
#pragma unroll
    for (int t = 0; t < NQT; ++t) qok[t] = q0 + 32 * t + l31 < nq;
    for (int i = tid; i < QROWS; i += 512) {
        const uint32_t q = q0 + i < nq ? q0 + i : 0;
        const float4 m = qmeta[q];
        qv[i] = make_float4((tau[q] - slack - m.z) * m.x, m.y, m.w, qmeta[nq + q].x);
    }
    __syncthreads();
    const int swz = (l31 >> 1) & 7;
    int w_sl[4];
#pragma unroll
    for (int st = 0; st < 4; ++st) w_sl[st] = l31 * 128 + (((2 * st + h) ^ swz) * 16);

    const uint64_t u0 = (uint64_t)rg * 8 + xcd, ustep = (uint64_t)rgn * 8;
    if (u0 >= nunit) return;
    const uint64_t my_units = (nunit - u0 + ustep - 1) / ustep;
    // this wave's rows of unit u: corpus tile 2 u + (wave >> 2), rows 32 (wave & 3) + l31 of it
    const uint32_t wtile = (uint32_t)wave >> 2, wrow = ((uint32_t)wave & 3) * 32;
    const int8_t* lane_base = corpus_q8 + ((tile_lo + wtile) * KC * 128 + wrow + l31) * 128 + h * 16;
    // (Hand-counted waits on loads the compiler does not track were measured here too: within 1 % — with two waves per
    // SIMD the compiler's conservative vmcnt(0) at the loop header costs nothing measurable.)
    auto frag = [&](uint64_t u, int c, int st) {
        const i32x4* p = reinterpret_cast<const i32x4*>(lane_base + ((u * 2 * KC + c) * 128) * 128 + st * 32);
        return NT ? __builtin_nontemporal_load(p) : *p;
    };
    i32x4 a[KC][4];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int st = 0; st < 4; ++st) a[c][st] = frag(u0, c, st);

    volatile uint64_t* pend = reinterpret_cast<volatile uint64_t*>(lds + WBYTES) + wave * kPend;
    uint32_t npend = 0;  // wave-uniform
    const float4* tm = tmeta + tile_lo + wtile;
    float4 tm_next = tm[u0 * 2];
    i32x16 acc[NQT];
    for (uint64_t n = 0; n < my_units; ++n) {
        const uint64_t u = u0 + n * ustep;
        const uint64_t un = n + 1 < my_units ? u + ustep : u;  // the last unit re-reads itself (discarded)
        const float4 tmv = tm_next;
        tm_next = tm[un * 2];
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[t][r] = 0;
        cs_static_for<0, KC>([&](auto CC) {
            constexpr int c = decltype(CC)::value;
            const char* wc = Wl + c * QROWS * 128;
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                i32x4 w[NQT];
#pragma unroll
                for (int t = 0; t < NQT; ++t) w[t] = *reinterpret_cast<const i32x4*>(wc + t * 32 * 128 + w_sl[st]);
#pragma unroll
                for (int t = 0; t < NQT; ++t) acc[t] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[c][st], w[t], acc[t], 0, 0, 0);
            }
            // the registers of stage c are free: the same stage of the next unit (fenced: hoisted above the MFMAs the
            // loads would need registers of their own)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int st = 0; st < 4; ++st) a[c][st] = frag(un, c, st);
            __builtin_amdgcn_sched_barrier(0);
        });
        // the last MFMAs' results are read below through inline asm the hazard recogniser does not see into
        asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" ::: "memory");
        cs_static_for<0, NQT>([&](auto TC) {
            constexpr int t = decltype(TC)::value;
            // I > T  <=>  I > floor(T) for an integer I; NaN (flagged tile or query) -> every row
            const float4 qm = qv[32 * t + l31];
            const float T = q8_threshold(qm.x, qm.y, qm.z, qm.w, tmv, kQ8Quarter * (float)DIM);
            const int Ti = (T == T) ? (T < -2.0e9f ? (int)0x80000000 : (T > 2.0e9f ? 0x7fffffff : (int)T)) : (int)0x80000000;
            const bool all = !(T == T) || T < -2.0e9f;
            // explicit reads: left to itself the compiler copies every accumulator out of the AGPRs in one block
            int v[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v[r]) : "a"(acc[t][r]));
            int top = v[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) top = v[r] > top ? v[r] : top;
            if (!__ballot(qok[t] && (all || top > Ti))) return;
            uint32_t hm = 0;  // a tile with a candidate (rare): sixteen pushes as ONE rolled loop over a hit mask
#pragma unroll
            for (int r = 0; r < 16; ++r) hm |= (uint32_t)(all || v[r] > Ti) << r;
#pragma nounroll
            for (int r = 0; r < 16; ++r) {
                const uint64_t m = u * 256 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                cand_push(qok[t] && m < M && ((hm >> r) & 1u), q0 + 32 * t + l31, row_lo + m, dead, pend, npend, lane, cand,
                          cnt, cap);
            }
        });
    }
    cand_flush(pend, npend, lane, cand, cnt, cap);
}

// ---- host side ----------------------------------------------------------------------------

bool split_scan_supported(uint32_t dim) { return dim == 384 || dim == 768 || dim == 1024; }

static int32_t launch_unit_f16(const float* d_src, const float* d_norm, _Float16* d_dst, uint64_t rows, uint32_t dim,
                               hipStream_t stream, int tiled = 0, uint64_t dst_row0 = 0) {
    const uint64_t n8 = rows * (dim / 8);
    if (n8 == 0) return CS_OK;
    const uint64_t want = (n8 + 255) / 256;
    hipLaunchKernelGGL(unit_f16_rows_kernel, dim3((uint32_t)(want < 8192 ? want : 8192)), dim3(256), 0, stream, d_src,
                       d_norm, d_dst, n8, dim, tiled, dst_row0);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_corpus_split(const float* d_corpus, const float* d_norms, _Float16* d_split, uint64_t first,
                            uint64_t n, uint32_t dim, hipStream_t stream) {
    return launch_unit_f16(d_corpus + first * dim, d_norms + first, d_split, n, dim, stream, 1, first);
}

int32_t launch_unit_mean(const float* d_corpus, const float* d_norms, uint64_t n, uint32_t dim, float* d_mu,
                         hipStream_t stream) {
    if (dim > 1024) return fail(CS_ERR_UNSUPPORTED, "int8 filter copy supports dim <= 1024, got %u", dim);
    CS_HIP(hipMemsetAsync(d_mu, 0, dim * sizeof(float), stream));
    if (n == 0) return CS_OK;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(n, 4096);
    hipLaunchKernelGGL(unit_mean_kernel, dim3(blocks), dim3(256), 0, stream, d_corpus, d_norms, n, dim, d_mu);
    CS_HIP(hipGetLastError());
    hipLaunchKernelGGL(mean_finish_kernel, dim3((dim + 255) / 256), dim3(256), 0, stream, d_mu, dim, 1.0f / (float)n);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_corpus_q8(const float* d_corpus, const float* d_norms, int8_t* d_q8, float4* d_tmeta, uint64_t first_tile,
                         uint64_t ntiles, uint32_t dim, const float* d_mu, hipStream_t stream) {
    for (uint64_t t = 0; t < ntiles;) {  // grid.x stays below 2^31
        const uint32_t n = (uint32_t)std::min<uint64_t>(ntiles - t, 1u << 30);
        if (dim == 384) hipLaunchKernelGGL(corpus_q8_kernel<3>, dim3(n), dim3(256), 0, stream, d_corpus, d_norms, d_q8, d_tmeta, first_tile + t, d_mu);
        else if (dim == 768) hipLaunchKernelGGL(corpus_q8_kernel<6>, dim3(n), dim3(256), 0, stream, d_corpus, d_norms, d_q8, d_tmeta, first_tile + t, d_mu);
        else if (dim == 1024) hipLaunchKernelGGL(corpus_q8_kernel<8>, dim3(n), dim3(256), 0, stream, d_corpus, d_norms, d_q8, d_tmeta, first_tile + t, d_mu);
        else return fail(CS_ERR_UNSUPPORTED, "int8 filter copy supports dim 384/768/1024, got %u", dim);
        CS_HIP(hipGetLastError());
        t += n;
    }
    return CS_OK;
}

// The laboratory knobs of the filter plan (filter_plan.hpp), read once; in the product library they are the defaults.
const FilterKnobs& filter_knobs() {
    static const FilterKnobs kn = [] {
        FilterKnobs d;
        const auto num = [](const char* name, auto& v) {
            if (const char* e = cs_lab_env(name)) v = (std::decay_t<decltype(v)>)std::atoi(e);
        };
        const auto real = [](const char* name, double& v) {
            if (const char* e = cs_lab_env(name)) v = std::atof(e);
        };
        const auto on = [](const char* name, bool& v) {
            if (const char* e = cs_lab_env(name)) v = e[0] != '0';
        };
        num("CS_FILTER_INT8_MAX_Q", d.int8_max_q);
        num("CS_FILTER_INT8_RW_MAX_Q", d.int8_rw_max_q);
        on("CS_FILTER_INT8_RQ", d.int8_rq);
        num("CS_FILTER_INT8_Q2", d.int8_q2);
        num("CS_FILTER_WIDE_MIN_Q", d.wide_min_q);
        num("CS_FILTER_RW", d.rw);
        num("CS_FILTER_GROWTH", d.growth);
        if (d.growth == 1) d.growth = 2;
        num("CS_FILTER_GROWTH1", d.growth1);
        real("CS_FILTER_GMAX", d.gmax);
        real("CS_FILTER_G1MAX", d.g1max);
        num("CS_FILTER_G1_MAXQ", d.g1_maxq);
        real("CS_FILTER_G1_CAND", d.g1_cand);
        on("CS_FILTER_INT8_RW256", d.int8_rw256);
        on("CS_FILTER_NT", d.nt);
        num("CS_FILTER_PHASE0_BLOCKS", d.phase0_blocks);
        return d;
    }();
    return kn;
}

// The filter instantiations scan_split_impl<J> can launch, as (kernel, 32-query groups per tile).  Their dynamic-LDS
// limits are set from this list and a launch finds its kernel in it, so no instantiation runs without its limit.
struct FilterInst {
    FilterKernel kernel;
    uint32_t nqt;
};
template <int J>
constexpr auto filter_insts() {
    using K = FilterKernel;
    if constexpr (J == 3)
        return std::array<FilterInst, 14>{{{K::F16Tile128, 0}, {K::F16Tile256, 0}, {K::Q8Tile256, 0}, {K::F16Rw, 1},
                                           {K::F16Rw, 2}, {K::F16Rw, 4}, {K::Q8Rw, 1}, {K::Q8Rw, 2}, {K::Q8Rw, 4},
                                           {K::Q8Rw, 8}, {K::Q8Rw2, 1}, {K::Q8Rw2, 2}, {K::Q8Rq, 8}, {K::Q8Rq1, 8}}};
    else if constexpr (J == 6)
        return std::array<FilterInst, 10>{{{K::F16Tile128, 0}, {K::F16Tile256, 0}, {K::Q8Tile256, 0}, {K::F16Rw, 1},
                                           {K::F16Rw, 2}, {K::Q8Rw, 1}, {K::Q8Rw, 2}, {K::Q8Rw, 4}, {K::Q8Rw2, 1},
                                           {K::Q8Rw2, 2}}};
    else
        return std::array<FilterInst, 6>{{{K::F16Tile128, 0}, {K::F16Tile256, 0}, {K::Q8Tile256, 0}, {K::F16Rw, 1},
                                          {K::Q8Rw, 1}, {K::Q8Rw, 2}}};
}

template <class Fn>
struct FilterFn {
    Fn fn;
    size_t lds;  // dynamic LDS bytes
};
template <class Fn>
FilterFn(Fn, size_t) -> FilterFn<Fn>;

// entry I of filter_insts<J>(): the kernel and its dynamic LDS
template <int J, size_t I>
static auto filter_fn() {
    constexpr FilterInst f = filter_insts<J>()[I];
    constexpr int N = (int)f.nqt;
    using K = FilterKernel;
    if constexpr (f.kernel == K::F16Tile128) return FilterFn{&score_filter_kernel, (size_t)SH_LDS_BYTES};
    else if constexpr (f.kernel == K::F16Tile256) return FilterFn{&score_filter256p_kernel<false>, (size_t)UF2_LDS};
    else if constexpr (f.kernel == K::Q8Tile256) return FilterFn{&score_filter256p_kernel<true>, (size_t)UF2_LDS};
    else if constexpr (f.kernel == K::F16Rw) return FilterFn{&score_filter_rw_kernel<N, 2 * J>, (size_t)RwGeom<N, 2 * J>::LDS_ALL};
    else if constexpr (f.kernel == K::Q8Rw) return FilterFn{&score_filter_rw8_kernel<N, J>, (size_t)Rw8Geom<N, J>::LDS_ALL};
    else if constexpr (f.kernel == K::Q8Rw2)
        return FilterFn{&score_filter_rw8_kernel<N, J, true>, (size_t)Rw8GeomT<N, J, true>::LDS_ALL};
    else return FilterFn{&score_filter_rq8_kernel<N, J, f.kernel == K::Q8Rq1>, (size_t)kRq8Lds<N, J>};
}

template <int J, class F, size_t... I>
static void for_each_filter(F&& f, std::index_sequence<I...>) {
    (f(std::integral_constant<size_t, I>{}), ...);
}
template <int J, class F>
static void for_each_filter(F&& f) {
    for_each_filter<J>(f, std::make_index_sequence<filter_insts<J>().size()>{});
}

static_assert(UF2_BM == 256 && UF2_BN == 256 && SH_BM == 128 && SH_BN == 128, "filter_plan.hpp's tile sizes");

// The dynamic-LDS limits of every instantiation of filter_insts<J>(), once per device: before the first launch of any of them.
template <int J>
static int32_t filter_attributes() {
    static PerDeviceOnce attr_set;  // function attributes are per device
    return attr_set.run([&]() -> int32_t {
        hipError_t e = hipSuccess;
        for_each_filter<J>([&](auto i) {
            const auto f = filter_fn<J, i>();
            if (e == hipSuccess)
                e = hipFuncSetAttribute(reinterpret_cast<const void*>(f.fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)f.lds);
        });
        CS_HIP(e);
        return CS_OK;
    });
}

template <int J>
static int32_t prep_queries_impl(const BatchedState& st, const SplitQueryWs& qw, const float* d_queries, uint32_t nq, uint32_t k,
                                 uint32_t first_rows, const float* d_mu, bool use_q8, bool two_planes, hipStream_t stream) {
    hipLaunchKernelGGL(prep_queries_kernel<J>, dim3((nq + 7) / 8), dim3(256), 0, stream,
                       qw.q_pinned ? qw.q_pinned : d_queries, qw.q_pinned ? const_cast<float*>(d_queries) : nullptr, nq,
                       qw.d_qmag, qw.d_qsplit, st.d_tau, st.d_cnt, st.d_carry, k, st.d_overflow, first_rows,
                       use_q8 ? qw.d_q8q : nullptr, qw.d_qmeta, use_q8 ? d_mu : nullptr, st.h_mirror,
                       two_planes ? qw.d_q8q_hi : nullptr, qw.d_q8q_lo);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_prep_queries(uint32_t dim, const BatchedState& st, const SplitQueryWs& qw, const float* d_queries, uint32_t nq,
                            uint32_t k, uint32_t first_rows, const float* d_mu, bool use_q8, bool two_planes, hipStream_t stream) {
    const auto impl = dim == 384 ? prep_queries_impl<3> : dim == 768 ? prep_queries_impl<6> : dim == 1024 ? prep_queries_impl<8> : nullptr;
    if (!impl) return fail(CS_ERR_UNSUPPORTED, "split scan supports dim 384/768/1024, got %u", dim);
    return impl(st, qw, d_queries, nq, k, first_rows, d_mu, use_q8, two_planes, stream);
}

// One phase's filter launch and the int8 tail behind it, as planned.
template <int J>
static int32_t filter_phase_impl(const FilterPhase& ph, const FilterOperands& op) {
    constexpr uint32_t dim = 128 * J;
    CS_TRY(filter_attributes<J>());
    const BatchedState& st = *op.st;
    const SplitQueryWs& qw = *op.qw;
    const Q8View* q8 = op.q8;
    const _Float16* d_split = op.d_split;
    const uint32_t* d_dead = op.d_dead;
    const uint32_t nq = op.nq, cap = op.cap, nt = op.nt_stream;
    const float margin = op.margin;
    hipStream_t stream = op.stream;
    uint32_t* cand = reinterpret_cast<uint32_t*>(st.d_cand);
    using K = FilterKernel;
    if (ph.kernel != K::None) {
        // what the kernels take for granted (plan_filter and scoped_filter_plan.hpp keep to it)
        const bool i8 = ph.kernel == K::Q8Tile256 || ph.kernel == K::Q8Rq || ph.kernel == K::Q8Rq1 || ph.kernel == K::Q8Rw || ph.kernel == K::Q8Rw2;
        const bool resident = ph.kernel != K::Q8Tile256 && ph.kernel != K::F16Tile256 && ph.kernel != K::F16Tile128;
        bool found = false;
        for_each_filter<J>([&](auto i) {
            constexpr FilterInst f = filter_insts<J>()[i];
            found = found || (ph.kernel == f.kernel && ph.nqt == f.nqt);
        });
        if (!found) return fail(CS_ERR_BAD_ARG, "filter phase: no kernel %d with %u query groups at dim %u", (int)ph.kernel, ph.nqt, dim);
        if (ph.lo % 128 || (i8 && ph.filter_hi % 128))
            return fail(CS_ERR_BAD_ARG, "filter phase: rows [%llu, %llu) are not whole 128-row tiles", (unsigned long long)ph.lo,
                        (unsigned long long)(i8 ? ph.filter_hi : ph.hi));
        if (resident && (ph.qtiles == 0 || ph.grid % 8 || ph.grid < 8 * ph.qtiles))
            return fail(CS_ERR_BAD_ARG, "filter phase: a resident-query grid is a multiple of 8, at least 8 per query tile (grid %u, %u query tiles)",
                        ph.grid, ph.qtiles);
        if (ph.grid == 0 || nq == 0 || (i8 ? !(q8 && q8->d_q8 && q8->d_tmeta && qw.d_q8q && qw.d_qmeta) : !(d_split && qw.d_qsplit)) ||
            (ph.kernel == K::Q8Rw2 && !(qw.d_q8q_hi && qw.d_q8q_lo)))
            return fail(CS_ERR_BAD_ARG, "filter phase: no grid, no queries or no operands for kernel %d", (int)ph.kernel);
    }
    for_each_filter<J>([&](auto i) {
        constexpr FilterInst f = filter_insts<J>()[i];
        if (ph.kernel != f.kernel || ph.nqt != f.nqt) return;
        const auto k = filter_fn<J, i>();
        if constexpr (f.kernel == K::F16Tile128)
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(256), k.lds, stream, d_split, ph.lo, ph.hi, dim / 64, qw.d_qsplit, nq,
                               st.d_tau, d_dead, cand, st.d_cnt, cap, margin);
        else if constexpr (f.kernel == K::F16Tile256)
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(512), k.lds, stream, d_split, ph.lo, ph.hi, dim / 64, qw.d_qsplit, nq,
                               st.d_tau, d_dead, cand, st.d_cnt, cap, ph.slots, margin, (const float4*)nullptr,
                               (const float4*)nullptr);
        else if constexpr (f.kernel == K::Q8Tile256)
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(512), k.lds, stream, reinterpret_cast<const _Float16*>(q8->d_q8), ph.lo,
                               ph.filter_hi, dim / 128, reinterpret_cast<const _Float16*>(qw.d_q8q), nq, st.d_tau, d_dead,
                               cand, st.d_cnt, cap, ph.slots, q8_slack(dim), q8->d_tmeta, qw.d_qmeta);
        else if constexpr (f.kernel == K::F16Rw)
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(256), k.lds, stream, d_split, ph.lo, ph.hi, qw.d_qsplit, nq, st.d_tau,
                               d_dead, cand, st.d_cnt, cap, ph.qtiles, nt, margin);
        else if constexpr (f.kernel == K::Q8Rw || f.kernel == K::Q8Rw2)
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(256), k.lds, stream, q8->d_q8, q8->d_tmeta, ph.lo, ph.filter_hi,
                               f.kernel == K::Q8Rw2 ? qw.d_q8q_hi : qw.d_q8q, qw.d_qmeta, nq, st.d_tau, d_dead, cand,
                               st.d_cnt, cap, ph.qtiles, nt, q8_slack(dim), f.kernel == K::Q8Rw2 ? qw.d_q8q_lo : nullptr);
        else
            hipLaunchKernelGGL(k.fn, dim3(ph.grid), dim3(512), k.lds, stream, q8->d_q8, q8->d_tmeta, ph.lo, ph.filter_hi,
                               qw.d_q8q, qw.d_qmeta, nq, st.d_tau, d_dead, cand, st.d_cnt, cap, ph.qtiles, q8_slack(dim));
    });
    if (ph.tail_hi > ph.tail_lo)  // fewer than 128 rows behind the int8 copy's last complete tile
        hipLaunchKernelGGL(tail_candidates_kernel, dim3(nq), dim3(128), 0, stream, ph.tail_lo, ph.tail_hi, d_dead, cand,
                           st.d_cnt, cap);
    return CS_OK;
}

int32_t launch_filter_phase(uint32_t dim, const FilterPhase& ph, const FilterOperands& op) {
    const auto impl = dim == 384 ? filter_phase_impl<3> : dim == 768 ? filter_phase_impl<6> : dim == 1024 ? filter_phase_impl<8> : nullptr;
    if (!impl) return fail(CS_ERR_UNSUPPORTED, "split scan supports dim 384/768/1024, got %u", dim);
    return impl(ph, op);
}

// Launches what plan_filter plans: prep, then per phase the filter kernel, the int8 tail, the exact re-score and the select.
template <int J>
static int32_t scan_split_impl(const BatchedState& st, const SplitQueryWs& qw, const float* d_corpus,
                               const _Float16* d_split, uint64_t n_rows, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead,
                               RowIds id_base, uint64_t* d_out_keys, float* d_out_cos,
                               uint32_t* d_out_ids, uint32_t* d_out_counts, hipStream_t stream, float margin,
                               const Q8View* q8, const FilterPlan* prepared, const uint32_t* d_phase0_list,
                               const SimilarRefine* similar) {
    constexpr uint32_t dim = 128 * J;
    const uint32_t cap = batched_cap(k);
    CS_TRY(filter_attributes<J>());
    const FilterKnobs& kn = filter_knobs();
    const bool q8_ready = q8 && q8->d_q8 && qw.d_q8q && qw.d_qmeta;
    // a prepared plan (a scoped search: scoped_filter_plan.hpp) is launched as it stands: its phase 0 are the first
    // phase0_rows entries of d_phase0_list, and d_dead is the scope's blocked-rows bitmap
    if (prepared && !(q8_ready && d_phase0_list && d_dead && prepared->use_q8 && (!prepared->two_planes || (qw.d_q8q_hi && qw.d_q8q_lo))))
        return fail(CS_ERR_BAD_ARG, "a prepared filter plan needs the int8 copy, its query planes, a bitmap and a phase-0 list");
    const FilterPlan plan = prepared ? *prepared
                                     : plan_filter(dim, n_rows, nq, k, q8_ready ? q8->rows : 0, qw.d_q8q_hi && qw.d_q8q_lo, cu_count(), kn);
    CS_TRY(prep_queries_impl<J>(st, qw, d_queries, nq, k, plan.phase0_rows, q8 ? q8->d_mu : nullptr, plan.use_q8, plan.two_planes, stream));
    FilterOperands op;
    op.st = &st; op.qw = &qw; op.d_split = d_split; op.q8 = q8; op.d_dead = d_dead;
    op.nq = nq; op.cap = cap; op.margin = margin; op.nt_stream = kn.nt; op.stream = stream;
    for (uint32_t p = 0; p < plan.nphases; ++p) {
        const FilterPhase& ph = plan.phase[p];
        CS_TRY(filter_phase_impl<J>(ph, op));
        const bool first = ph.lo == 0, last = p + 1 == plan.nphases;  // (plan_filter: the phase that reaches n_rows)
        if (ph.hi > ph.lo && !first) CS_HIP(hipGetLastError());
        if (similar) {  // a similar-chunk search: its own refine and fold (scan_similar_filter.hip), same grids
            // (a prepared plan's phase 0 is phase0_rows list entries; ph.hi is then a row boundary, not a count)
            CS_TRY(launch_similar_rescore(st, qw, d_corpus, dim, d_queries, nq, cap, ph.rk_blocks,
                                          first ? (prepared ? plan.phase0_rows : (uint32_t)ph.hi) : 0u, d_dead, id_base, similar->gv,
                                          similar->sv, stream, prepared ? d_phase0_list : nullptr));
            CS_TRY(launch_similar_select(st, nq, cap, k, last, similar->sv, d_out_keys, d_out_cos, d_out_ids, d_out_counts, stream));
            continue;
        }
        if (first && prepared)
            hipLaunchKernelGGL((rescore_keys_kernel<J, true>), dim3(ph.rk_blocks, nq), dim3(RK_THREADS), 0, stream, d_corpus,
                               d_queries, qw.d_qmag, st.d_cand, st.d_cnt, cap, id_base, plan.phase0_rows, d_phase0_list);
        else
            hipLaunchKernelGGL(rescore_keys_kernel<J>, dim3(ph.rk_blocks, nq), dim3(RK_THREADS), 0, stream, d_corpus, d_queries,
                               qw.d_qmag, st.d_cand, st.d_cnt, cap, id_base, first ? (uint32_t)ph.hi : 0u, d_dead);
        CS_HIP(hipGetLastError());
        CS_TRY(launch_select_candidates(st, nq, cap, k, last, d_out_keys, d_out_cos, d_out_ids, d_out_counts, stream));
    }
    return CS_OK;
}

int32_t launch_scan_split(const BatchedState& st, const SplitQueryWs& qw, const float* d_corpus,
                          const _Float16* d_split, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead,
                          RowIds id_base, uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                          uint32_t* d_out_counts, hipStream_t stream, float margin, const Q8View* q8,
                          const FilterPlan* prepared, const uint32_t* d_phase0_list, const SimilarRefine* similar) {
    const auto impl = dim == 384 ? scan_split_impl<3> : dim == 768 ? scan_split_impl<6> : dim == 1024 ? scan_split_impl<8> : nullptr;
    if (!impl) return fail(CS_ERR_UNSUPPORTED, "split scan supports dim 384/768/1024, got %u", dim);
    return impl(st, qw, d_corpus, d_split, n_rows, d_queries, nq, k, d_dead, id_base, d_out_keys, d_out_cos, d_out_ids,
                d_out_counts, stream, margin, q8, prepared, d_phase0_list, similar);
}

}  // namespace cs
