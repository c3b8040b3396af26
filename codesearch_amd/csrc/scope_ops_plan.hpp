// scope_ops_plan.hpp — the arithmetic of scope algebra (scope_ops.hip; index.hip cs_scope_combine): union, intersection
// and difference of two strictly ascending u32 id sets by merge path.  Everything here is __host__ __device__ or plain
// host C++17: tests/cpp/scope_ops_plan_test.cpp walks the very functions the kernels call, tile by tile, on the CPU.
//
// THE MERGED SEQUENCE of a[0, na) and b[0, nb) orders all na + nb elements ascending; on equal ids the element of a goes
// before the element of b (the tie rule).  It is never materialised.  Position d of it (a DIAGONAL, 64-bit: na + nb can
// pass 2^32) splits into i elements of a and d - i of b: merge_split finds i by bisection.
//
// A TILE is kScopeOpsTile consecutive positions; one block owns one tile, one thread kScopeOpsPerThread consecutive
// positions of it (scope_ops_walk).  What an element needs to know beyond itself is one neighbour:
//   - an element of b is a DUPLICATE exactly when it equals the element of a placed just before it, a[i - 1] with i the
//     a-cursor at that moment (every a[< i] <= it was placed before it, a[i - 1] is the largest of them);
//   - an element of a HAS A TWIN exactly when it equals the next element of b, b[j] with j the b-cursor at that moment
//     (the twin, if any, follows it immediately: ties put a first and b is strictly ascending).
// Either neighbour may lie outside the tile's slices: a[i0 - 1] belongs to the previous tile, b[j1] to the next.  A
// slice therefore carries them: the a-slice one element in FRONT (valid when i0 > 0), the b-slice one BEHIND (valid when
// j1 < nb), both re-read from HBM by the block that needs them.
//   union         keeps every a and every b that is no duplicate
//   intersection  keeps the b that are duplicates
//   difference    keeps the a that have no twin
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define CS_SCOPE_OPS_HD __host__ __device__ __forceinline__
#else
#define CS_SCOPE_OPS_HD inline
#endif

namespace cs {

constexpr uint32_t kScopeOpsBlock = 256;      // threads of a set-operation block
constexpr uint32_t kScopeOpsPerThread = 16;   // merged positions one thread walks
constexpr uint32_t kScopeOpsTile = kScopeOpsBlock * kScopeOpsPerThread;  // 4,096 positions: cs_scope_ops_tile()

constexpr int32_t kScopeOpUnion = 0, kScopeOpIntersect = 1, kScopeOpDifference = 2;  // CS_SCOPE_OP_*

// The elements of a among the first d of the merged sequence, 0 <= d <= na + nb: the smallest i with
// !(a[i] <= b[d - 1 - i]).  Reads a[i] for i < min(d, na) and b[j] for j < min(d, nb) only.
CS_SCOPE_OPS_HD uint64_t merge_split(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb, uint64_t d) {
    uint64_t lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] <= b[d - 1 - mid]) lo = mid + 1;  // a[mid] goes before b[d - 1 - mid]: it is among the first d
        else hi = mid;
    }
    return lo;
}

// Tiles of the merged sequence of na + nb elements.
CS_SCOPE_OPS_HD uint64_t scope_ops_tiles(uint64_t na, uint64_t nb) { return (na + nb + kScopeOpsTile - 1) / kScopeOpsTile; }

CS_SCOPE_OPS_HD bool scope_ops_keep_a(int32_t op, uint32_t x, bool next_valid, uint32_t b_next) {
    if (op == kScopeOpUnion) return true;
    if (op == kScopeOpIntersect) return false;
    return !(next_valid && b_next == x);
}

CS_SCOPE_OPS_HD bool scope_ops_keep_b(int32_t op, uint32_t y, bool prev_valid, uint32_t a_prev) {
    const bool dup = prev_valid && a_prev == y;
    if (op == kScopeOpUnion) return !dup;
    if (op == kScopeOpIntersect) return dup;
    return false;
}

// One thread's walk: `steps` <= kScopeOpsPerThread positions of a tile, starting with ia elements of the a-slice and ib of
// the b-slice behind it.  A[0, na) and B[0, nb) are the tile's slices; A[-1] is readable when has_prev (a[i0 - 1]), B[nb]
// when has_next (b[j1]).  vals[s] = the element at step s, bit s of the result set when the operation keeps it.
CS_SCOPE_OPS_HD uint32_t scope_ops_walk(int32_t op, const uint32_t* A, uint32_t na, bool has_prev, const uint32_t* B, uint32_t nb,
                                        bool has_next, uint32_t ia, uint32_t ib, uint32_t steps,
                                        uint32_t (&vals)[kScopeOpsPerThread]) {
    uint32_t kept = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t s = 0; s < kScopeOpsPerThread; ++s) {
        vals[s] = 0;
        if (s >= steps) continue;
        const bool from_a = ia < na && (ib >= nb || A[ia] <= B[ib]);
        bool keep;
        if (from_a) {
            const uint32_t x = A[ia];
            const bool next_valid = ib < nb || has_next;
            keep = scope_ops_keep_a(op, x, next_valid, next_valid ? B[ib] : 0u);
            vals[s] = x;
            ++ia;
        } else {
            const uint32_t y = B[ib];
            const bool prev_valid = ia > 0 || has_prev;
            keep = scope_ops_keep_b(op, y, prev_valid, prev_valid ? A[(int32_t)ia - 1] : 0u);
            vals[s] = y;
            ++ib;
        }
        kept |= (keep ? 1u : 0u) << s;
    }
    return kept;
}

// ---- striped shards: a range of global ids, and a part's local ids back to global ones ----------------------------
// The global ids below g that shard s of n holds under stripes of `stripe` ids.  A shard's local ids are dense, so this is
// also the local id of g on its own shard, and [below(first), below(first + n)) is the local range of a global range.
inline uint64_t shard_ids_below(uint64_t g, uint64_t stripe, uint32_t nshards, uint32_t s) {
    const uint64_t full = g / stripe;  // whole stripes below g
    uint64_t cnt = full > s ? (full - s + nshards - 1) / nshards * stripe : 0;
    if (full % nshards == s) cnt += g % stripe;
    return cnt;
}

inline uint64_t shard_global_id(uint64_t local, uint64_t stripe, uint32_t nshards, uint32_t s) {
    return ((local / stripe) * nshards + s) * stripe + local % stripe;
}

}  // namespace cs
