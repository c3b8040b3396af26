// scan_wave.hpp — the shared body of the cosine scans.  The streaming scan (scan.hip), the gathered scan over a row list
// (scan_masked.hip) and the capped scan (scan_grouped.hip) all score a row with the functions of this file — query
// fragments and mag_a, the per-row fmaf chains and mag_b, the zero guard and the divide — and select with its lists, its
// prime-pass tail and its block merge, so "the streaming scan's cosine bits" holds by construction, not by three texts kept
// equal.  A kernel adds only what makes it that kernel: how a tile's rows are addressed, cached or non-temporal loads, the
// gate, tombstones, the group slots.
#pragma once

#include "common.hpp"
#include "search_route.hpp"  // kScanWaves

namespace cs {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kBlock = 256;   // 4 waves
constexpr int kWaves = kBlock / 64;
static_assert(kWaves == (int)kScanWaves, "search_route.hpp sizes the prime sample by it");

// ---- wave helpers ---------------------------------------------------------------------

// Sum over the 32 lanes of each half-wave; every lane of the half receives the total.
__device__ __forceinline__ float half_allreduce_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}
__device__ __forceinline__ float wave_allreduce_sum(float v) {
    v += __shfl_xor(v, 32, 64);
    return half_allreduce_sum(v);
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
    lo = __shfl_xor(lo, m, 64);
    hi = __shfl_xor(hi, m, 64);
    return ((uint64_t)hi << 32) | lo;
}

// thr / wpos of a wave's list[0, k) once every slot has been written: the worst key (the smallest packed key; an empty
// slot, 0, before any key; the lowest slot among equals) and its slot, by a 64-lane search (~1,000 cycles at k = 200).
// thr = floor while a slot is empty.  FULL: the caller knows that none is (a list filled by counting its inserts).
typedef volatile uint64_t __attribute__((address_space(3))) lds_vu64;
template <bool FULL = false>
__device__ __forceinline__ void wave_list_worst(lds_vu64* list, uint32_t k, int lane, float& thr, uint32_t& wpos,
                                                float floor = -__builtin_huge_valf()) {
    uint64_t mk = ~0ull;
    uint32_t mp = 0xffffffffu;
    for (uint32_t i = lane; i < k; i += 64) {
        uint64_t v = list[i];
        if (v < mk) { mk = v; mp = i; }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        uint64_t ok = shfl_xor_u64(mk, m);
        uint32_t op = __shfl_xor(mp, m, 64);
        if (ok < mk || (ok == mk && op < mp)) { mk = ok; mp = op; }
    }
    wpos = mp | 0x80000000u;
    thr = (!FULL && mk == 0ull) ? floor : key_cos(mk);
}

// Per-wave candidate list: k live slots (of kpad) in LDS holding packed keys, 0 = empty.
// State kept by the caller: `thr` = cosine of the current worst slot (-inf while any slot
// is empty) and `wpos` = that slot's index.  Rows are streamed in ascending id, so a row
// that ties the worst cosine loses to it (id asc) and `c > thr` is the whole test — the
// `>` of benchmark_models.rs:160.  `floor` is what thr falls back to while a slot is empty:
// -inf, or the primed lower bound (see scan_topk_kernel's PRIME mode).
__device__ __forceinline__ void wave_list_insert(volatile uint64_t* list_generic, uint32_t k, int lane,
                                                 float c, uint32_t id, float& thr,
                                                 uint32_t& wpos,
                                                 float floor = -__builtin_huge_valf()) {
    // While the list still has empty slots they are filled in index order (the search below picks the lowest
    // empty slot), thr stays at the floor and nothing needs searching: wpos < kListFull counts the filled slots.
    // A k = 200 list over a small corpus never leaves this phase; the 64-lane search starts with the insert that
    // fills the last slot.
    constexpr uint32_t kListFull = 0x80000000u;
    const uint32_t slot = wpos & ~kListFull;
    // The list is LDS; say so.  Through the generic pointer these were flat_store / flat_load, which count on vmcnt
    // as well and return out of order with the corpus loads in flight: every `s_waitcnt vmcnt(N)` of the scan loop
    // after a possible insert degraded to vmcnt(0).
    lds_vu64* const list = (lds_vu64*)list_generic;
    if (lane == 0) list[slot] = key_pack(c, id);
    if (!(wpos & kListFull) && slot + 1 < k) {
        wpos = slot + 1;
        return;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    wave_list_worst(list, k, lane, thr, wpos, floor);
}

// Bitonic sort, descending, of a[0..n) (n a power of two) by all threads of the block.
// Pair t of a stage is handled by thread t % T, i.e. by wave (t / 64) % (T / 64), and for strides
// <= 64 it lies inside the 128-key segment [128 (t / 64), +128): such a stage reads only what the
// same wave wrote in the stage before, so it needs the wave's own LDS ordering, not a block
// barrier.  Only stages with stride >= 128, and the stage right after one, synchronise the block
// (20 of the 78 stages of a 4096-key sort).
template <int T>
__device__ __forceinline__ void block_bitonic_desc(uint64_t* a, uint32_t n, int tid) {
    uint32_t prev_stride = 128;  // whatever filled a[] was another wave
    for (uint32_t size = 2; size <= n; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            if (stride >= 128 || prev_stride >= 128) {
                __syncthreads();
            } else {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            prev_stride = stride;
            for (uint32_t t = tid; t < (n >> 1); t += T) {
                uint32_t i = 2 * t - (t & (stride - 1));
                uint32_t j = i + stride;
                uint64_t x = a[i], y = a[j];
                bool desc = ((i & size) == 0);
                if ((x < y) == desc) { a[i] = y; a[j] = x; }
            }
        }
    }
    __syncthreads();
}

__device__ __forceinline__ bool row_is_dead(const uint32_t* dead, uint64_t row) {
    if (!dead) return false;
    return (dead[row >> 5] >> (row & 31)) & 1u;
}

// ---- the row arithmetic ----------------------------------------------------------------------------------
// The fast kernels (dim = 128 * J): lane l32 of a half-wave holds columns [128 j + 4 l32, +4) of its row for j < J, QT
// queries are scored per pass from registers.  Everything below is exact about its order of operations: it IS the result.
// load_query_fragment and block_merge_store take ONE query and the kernels loop over the pass's queries around them: with
// the loop inside the helper the compiler numbers registers and orders two address computations differently in every
// fast kernel; in this form a change here can be checked against otherwise unchanged code objects
// (benchmarks/compare_device_code.py).

// batch.rs:320-323: zero magnitude -> 0.0, else dot / (mag_a * mag_b)
__device__ __forceinline__ float cosine_of(float d, float qmag, float xmag) {
    return (qmag == 0.0f || xmag == 0.0f) ? 0.0f : d / (qmag * xmag);
}

// Query q's fragments -> qf; returns its magnitude (mag_a of benchmark_models.rs:325).  The caller clamps q to nq - 1.
template <int J>
__device__ __forceinline__ float load_query_fragment(const float* __restrict__ queries, uint32_t q, int l32, f32x4 (&qf)[J]) {
    const f32x4* qp = reinterpret_cast<const f32x4*>(queries + (size_t)q * (128 * J)) + l32;
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        qf[j] = qp[j * 32];
        s = fmaf(qf[j].x, qf[j].x, s);
        s = fmaf(qf[j].y, qf[j].y, s);
        s = fmaf(qf[j].z, qf[j].z, s);
        s = fmaf(qf[j].w, qf[j].w, s);
    }
    return sqrtf(half_allreduce_sum(s));
}

// One row's fragments x against the QT queries: leaves this lane's share of every dot product in dot[] (the caller sums
// each over the half-wave) and returns mag_b.  Per j: the row's own squares first, then x, y, z, w per query.
template <int J, int QT>
__device__ __forceinline__ float row_products(const f32x4 (&x)[J], const f32x4 (&qf)[QT][J], float (&dot)[QT]) {
    float ss = 0.0f;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) dot[qi] = 0.0f;
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const f32x4 v = x[j];
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
    return sqrtf(half_allreduce_sum(ss));  // mag_b
}

// Any dim (e.g. the reference's own 4-d unit test, store.rs:846-893): one wave per row, lanes stride over columns.
// An exception to "every scan calls these": scan_grouped_generic_kernel carries the same lines itself, because with
// either function (or cosine_of alone) the compiler makes that kernel 2 instructions longer.  (The other exception is
// scan_masked_topk_kernel<8,2,4>, which carries load_query_fragment's, row_products' and cosine_of's: see there.)
__device__ __forceinline__ float wave_query_mag(const float* qp, uint32_t dim, int lane) {
    float s = 0.0f;
    for (uint32_t c = lane; c < dim; c += 64) s = fmaf(qp[c], qp[c], s);
    return sqrtf(wave_allreduce_sum(s));
}
__device__ __forceinline__ float wave_row_cosine(const float* xp, const float* qp, uint32_t dim, int lane, float qmag) {
    float ss = 0.0f, dot = 0.0f;
    for (uint32_t c = lane; c < dim; c += 64) {
        const float v = xp[c];
        ss = fmaf(v, v, ss);
        dot = fmaf(v, qp[c], dot);
    }
    const float xmag = sqrtf(wave_allreduce_sum(ss));
    return cosine_of(wave_allreduce_sum(dot), qmag, xmag);
}

// ---- the two tails ------------------------------------------------------------------------------------------

// End of a prime pass (scan.hip: "Primed scans").  thr[qi] holds each lane's running maximum.  Wave maxima -> HBM; the
// last block of the pass to finish picks the k-th largest per query and writes floor_out[q] = the float just below it (a
// bound in the denormal range becomes -FLT_MIN; -inf when fewer than k waves met a live row), then resets done_ctr.
// gw = this wave's index in the grid; lds_keys has room for kWaves * kpad keys and the host keeps the wave count under it.
template <int QT>
__device__ __forceinline__ void prime_pass_tail(const float (&thr)[QT], uint32_t q0, uint32_t nq, uint32_t k, uint64_t gw,
                                                int tid, int lane, uint64_t* lds_keys, float* __restrict__ wave_max,
                                                uint32_t* __restrict__ done_ctr, float* __restrict__ floor_out) {
    const uint32_t nwaves = gridDim.x * kWaves;
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
        const float m = fmaxf(__shfl(thr[qi], 0, 64), __shfl(thr[qi], 32, 64));
        if (lane == 0 && q0 + qi < nq)
            __hip_atomic_store(wave_max + (size_t)(q0 + qi) * nwaves + gw, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __shared__ uint32_t is_last;
    __threadfence();
    __syncthreads();
    if (tid == 0) {
        const uint32_t prev = __hip_atomic_fetch_add(done_ctr + blockIdx.y, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        is_last = (prev == gridDim.x - 1);
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    uint32_t nsort = 64;
    while (nsort < nwaves) nsort <<= 1;  // host keeps nsort <= kWaves * kpad (the LDS size)
#pragma unroll 1
    for (int qi = 0; qi < QT; ++qi) {
        if (q0 + qi >= nq) break;
        __syncthreads();
        for (uint32_t i = tid; i < nsort; i += kBlock) {
            float m = -__builtin_huge_valf();
            if (i < nwaves)
                m = __hip_atomic_load(wave_max + (size_t)(q0 + qi) * nwaves + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lds_keys[i] = (m == -__builtin_huge_valf()) ? 0ull : key_pack(m, 0u);
        }
        block_bitonic_desc<kBlock>(lds_keys, nsort, tid);
        if (tid == 0) {
            const uint64_t key = (k <= nsort) ? lds_keys[k - 1] : 0ull;
            float t = -__builtin_huge_valf();
            if (key) {
                const uint32_t o = (uint32_t)(key >> 32) - 1u;  // next float below the bound
                t = key_cos((uint64_t)o << 32);
                if (fabsf(t) < 1.17549435e-38f) t = -1.17549435e-38f;
            }
            floor_out[q0 + qi] = t;
        }
    }
    if (tid == 0) __hip_atomic_store(done_ctr + blockIdx.y, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Block merge of one query: its kWaves wave lists a[kWaves][kpad] -> best k, sorted, to partial[q][blockIdx.x][k].
__device__ __forceinline__ void block_merge_store(uint64_t* a, uint32_t kpad, uint32_t k, uint32_t q, int tid,
                                                  uint64_t* __restrict__ partial) {
    const uint32_t nsort = kWaves * kpad;
    block_bitonic_desc<kBlock>(a, nsort, tid);
    uint64_t* out = partial + ((size_t)q * gridDim.x + blockIdx.x) * k;
    for (uint32_t i = tid; i < k; i += kBlock) out[i] = a[i];
}

}  // namespace cs
