// scan_wave.hpp — wave and block helpers of the cosine scans: the streaming scan (scan.hip) and the masked scan over a
// row list (scan_masked.hip) share them, so both score and select with the same instructions.
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
    // A k = 200 list over a small corpus never leaves this phase; the 64-lane search (~1,000 cycles) starts with
    // the insert that fills the last slot.
    constexpr uint32_t kListFull = 0x80000000u;
    const uint32_t slot = wpos & ~kListFull;
    // The list is LDS; say so.  Through the generic pointer these were flat_store / flat_load, which count on vmcnt
    // as well and return out of order with the corpus loads in flight: every `s_waitcnt vmcnt(N)` of the scan loop
    // after a possible insert degraded to vmcnt(0).
    typedef volatile uint64_t __attribute__((address_space(3))) lds_vu64;
    lds_vu64* const list = (lds_vu64*)list_generic;
    if (lane == 0) list[slot] = key_pack(c, id);
    if (!(wpos & kListFull) && slot + 1 < k) {
        wpos = slot + 1;
        return;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
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
    wpos = mp | kListFull;
    thr = (mk == 0ull) ? floor : key_cos(mk);
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

}  // namespace cs
