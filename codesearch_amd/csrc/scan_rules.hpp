// scan_rules.hpp — the two selection rules that more than one scan file applies, stated once: the boost (scan_boosted.hip)
// and the capped wave list (scan_grouped.hip).  scan_boosted_grouped.hip applies both to the same row.  Device code only;
// the functions were moved here from those two files as they stood, and the files' code objects are what they were
// (benchmarks/compare_device_code.py; profiles/boosted_variants_device_code.log).
#pragma once

#include "scan.hpp"
#include "grouped_plan.hpp"
#include "scan_wave.hpp"

namespace cs {

// ---- the boost ------------------------------------------------------------------------------------------

// s of c: the reference's score
__device__ __forceinline__ float boosted_score(float c) { return 1.0f - (1.0f - c) * 0.5f; }
// An upper bound of fl(s * w) over every weight a row can take, wmin <= w <= wmax: the pre-gate's value
__device__ __forceinline__ float boosted_bound(float s, float wmin, float wmax) { return s * (s < 0.0f ? wmin : wmax); }

// The weight of the row that carries `id`: 1 without a class (ids past the table were appended after the last
// assignment; CS_NO_CLASS is past every table) or with a class the call's table does not cover.
__device__ __forceinline__ float boosted_weight(const BoostView& bv, uint32_t id) {
    const uint32_t i = id - bv.id_base;
    if (!bv.classes || i >= bv.len) return 1.0f;
    const uint32_t cls = bv.classes[i];
    return cls < bv.n_classes ? bv.weights[cls] : 1.0f;
}

// The stored row that carries `id`, which some stored row does: id - base under the identity numbering, else the
// position of id in the ascending table ids[0, n_rows).
__device__ __forceinline__ uint64_t boosted_row_of(const RowIds& row_ids, uint64_t n_rows, uint32_t id) {
    if (!row_ids.ids) return (uint64_t)(id - row_ids.base);
    uint64_t lo = 0, hi = n_rows;  // the first entry >= id
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (row_ids.ids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    return lo < n_rows ? lo : n_rows - 1;  // (a key always names a stored row; never read past the table)
}

// ---- the capped wave list ----------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;  // ids past the table (appended after the last assignment) are ungrouped
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

typedef volatile uint32_t __attribute__((address_space(3))) lds_vu32;

// wave_list_insert (scan_wave.hpp) under the cap.  `list` holds the capped top-k of the rows this wave has met, `glist`
// their groups; thr / wpos as there (wpos < 2^31 counts the filled slots of a list that is not full yet, thr = -inf then).
// The caller has established c > thr.  Rows arrive in ascending id, so a row that ties a key already there loses to it:
// packed keys compare that way by themselves (equal cosine, larger id -> smaller key).
//   group CS_NO_GROUP, or fewer than m slots hold g  -> the ordinary insert: next empty slot, or over the worst key;
//   m slots hold g                                   -> over the worst key OF GROUP g, and only if the row beats it.
// The slot search is skipped while fewer than m slots are filled at all: no group can be saturated yet.
// c is the value the list orders by: a cosine, or a boosted score (scan_boosted_grouped.hip).
__device__ __forceinline__ void wave_list_insert_grouped(volatile uint64_t* list_generic, volatile uint32_t* glist_generic,
                                                         uint32_t k, uint32_t m, int lane, float c, uint32_t id, uint32_t g,
                                                         float& thr, uint32_t& wpos) {
    constexpr uint32_t kListFull = 0x80000000u;
    lds_vu64* const list = (lds_vu64*)list_generic;
    lds_vu32* const glist = (lds_vu32*)glist_generic;
    const bool full = (wpos & kListFull) != 0;
    const uint32_t filled = full ? k : wpos;
    const uint64_t key = key_pack(c, id);
    if (g != kNoGroup && filled >= m) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t cnt = 0;
        uint64_t wk = ~0ull;
        uint32_t wp = 0xffffffffu;
        for (uint32_t i0 = 0; i0 < filled; i0 += 64) {
            const uint32_t i = i0 + lane;
            const bool hit = i < filled && glist[i] == g;
            cnt += (uint32_t)__popcll(__ballot(hit));
            if (hit) {
                const uint64_t v = list[i];
                if (v < wk) { wk = v; wp = i; }
            }
        }
        if (cnt >= m) {  // wave-uniform
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const uint64_t ok = shfl_xor_u64(wk, s);
                const uint32_t op = __shfl_xor(wp, s, 64);
                if (ok < wk || (ok == wk && op < wp)) { wk = ok; wp = op; }
            }
            if (key > wk) {
                if (lane == 0) list[wp] = key;  // the slot keeps its group
                if (full) {
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    wave_list_worst<true>(list, k, lane, thr, wpos);  // a full list has no empty slot
                }
            }
            return;
        }
    }
    const uint32_t slot = wpos & ~kListFull;
    if (lane == 0) {
        list[slot] = key;
        glist[slot] = g;
    }
    if (!full && slot + 1 < k) {
        wpos = slot + 1;
        return;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    wave_list_worst<true>(list, k, lane, thr, wpos);  // a full list has no empty slot
}

// A wave's list -> HBM, unsorted, empty slots as 0: list `blockIdx.x * kWaves + wave` of query q.
__device__ __forceinline__ void wave_list_store(const uint64_t* list, uint32_t k, int lane, uint64_t* __restrict__ partial,
                                                uint32_t q, int wave) {
    uint64_t* out = partial + ((size_t)q * (gridDim.x * kWaves) + (size_t)blockIdx.x * kWaves + wave) * k;
    for (uint32_t i = lane; i < k; i += 64) out[i] = list[i];
}

}  // namespace cs
