// scope_ops.hip — scope algebra on the device: the union, intersection or difference of two scopes' ascending id sets
// (index.hip cs_scope_combine), and the id set of a range (cs_index_scope_create_range).  Plan and arithmetic:
// scope_ops_plan.hpp, walked on the CPU by tests/cpp/scope_ops_plan_test.cpp.
//
// Merge path over the two d_ids arrays.  The merged sequence (ties: a before b) is cut into tiles of kScopeOpsTile
// positions, one block each.  A block
//   1. finds its two diagonal splits by bisection over a and b in HBM (threads 0 and 1: merge_split, 64-bit diagonals);
//   2. loads its slice of a and its slice of b into LDS with coalesced reads — at most kScopeOpsTile ids together;
//   3. every thread finds the split of its own diagonal inside the slices (merge_split again, over LDS) and walks
//      kScopeOpsPerThread positions (scope_ops_walk), keeping its elements and a keep-bit each in registers;
//   4. the keep counts are prefixed over the block (shuffle scan inside a wave, wave totals through LDS).
// Two passes in the discipline of the row-list making (scan_masked.hip part 4): the COUNT pass stops here and leaves the
// tile's count, mask_scan_kernel turns the counts into offsets and the total, the host reads the total back once and
// sizes the result, and the WRITE pass repeats 1-4, compacts the survivors into LDS in order and writes them with
// coalesced stores at the tile's offset.  No atomics: thread t's survivors precede thread t + 1's, tile t's precede
// tile t + 1's, so the output is ascending by construction.
//
// THE BOUNDARY CASE.  Whether an element of b is kept depends on the element of a placed just before it (equal: it is a
// duplicate), and whether an element of a survives a difference depends on the element of b behind it (equal: its twin).
// Ties put a first, so a tile boundary can fall between the two: the a element is the last position of tile t, its equal
// b element the first of tile t + 1.  Tile t + 1 then holds no element of a that could tell, and tile t no element of b.
// Each block therefore loads one id more on either side, straight from HBM: a[i0 - 1] in front of its a-slice when
// i0 > 0, and b[j1] behind its b-slice when j1 < nb (sA[0] and sB[nbt] below), and scope_ops_walk reads them exactly where
// a cursor stands at the slice's edge.  The same holds between two threads of one block, where the neighbour is simply
// the adjacent LDS word.
#include "scan.hpp"
#include "scope_ops_plan.hpp"

namespace cs {

constexpr uint32_t kScopeOpsWaves = kScopeOpsBlock / 64;

template <bool WRITE>
__global__ void __launch_bounds__(kScopeOpsBlock)
scope_ops_kernel(const uint32_t* __restrict__ a, uint64_t na, const uint32_t* __restrict__ b, uint64_t nb, int32_t op,
                 uint32_t* __restrict__ tiles, uint32_t* __restrict__ out, uint64_t out_cap) {
    __shared__ uint32_t sA[kScopeOpsTile + 1];  // [0] = a[i0 - 1], [1 + k] = a[i0 + k]; the WRITE pass stages its output here
    __shared__ uint32_t sB[kScopeOpsTile + 1];  // [k] = b[j0 + k], [nbt] = b[j1]
    __shared__ uint64_t split[2];
    __shared__ uint32_t wave_cnt[kScopeOpsWaves];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t total = na + nb;
    const uint64_t d0 = (uint64_t)blockIdx.x * kScopeOpsTile;
    const uint64_t d1 = d0 + kScopeOpsTile < total ? d0 + kScopeOpsTile : total;
    if (tid < 2) split[tid] = merge_split(a, na, b, nb, tid ? d1 : d0);
    __syncthreads();
    const uint64_t i0 = split[0], i1 = split[1], j0 = d0 - i0, j1 = d1 - i1;
    const uint32_t nat = (uint32_t)(i1 - i0), nbt = (uint32_t)(j1 - j0), len = (uint32_t)(d1 - d0);
    const bool has_prev = i0 > 0, has_next = j1 < nb;
    for (uint32_t k = tid; k < nat + 1; k += kScopeOpsBlock)
        if (k > 0 || has_prev) sA[k] = a[i0 + k - 1];
    for (uint32_t k = tid; k < nbt + 1; k += kScopeOpsBlock)
        if (k < nbt || has_next) sB[k] = b[j0 + k];
    __syncthreads();

    const uint32_t dt = tid * kScopeOpsPerThread < len ? tid * kScopeOpsPerThread : len;
    const uint32_t steps = len - dt < kScopeOpsPerThread ? len - dt : kScopeOpsPerThread;
    const uint32_t ia = (uint32_t)merge_split(sA + 1, nat, sB, nbt, dt);
    uint32_t vals[kScopeOpsPerThread];
    const uint32_t kept = scope_ops_walk(op, sA + 1, nat, has_prev, sB, nbt, has_next, ia, dt - ia, steps, vals);

    const uint32_t c = (uint32_t)__popc(kept);
    uint32_t x = c;  // inclusive scan inside the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        if (lane >= (uint32_t)d) x += y;
    }
    if (lane == 63) wave_cnt[wave] = x;
    __syncthreads();  // (also: every thread has finished reading sA and sB)
    uint32_t before = 0, sum = 0;
#pragma unroll
    for (uint32_t w = 0; w < kScopeOpsWaves; ++w) {
        before += w < wave ? wave_cnt[w] : 0u;
        sum += wave_cnt[w];
    }
    if (!WRITE) {
        if (tid == 0) tiles[blockIdx.x] = sum;
        return;
    }
    uint32_t at = before + x - c;
#pragma unroll
    for (uint32_t s = 0; s < kScopeOpsPerThread; ++s)
        if ((kept >> s) & 1u) sA[at++] = vals[s];
    __syncthreads();
    const uint64_t base = tiles[blockIdx.x];
    for (uint32_t k = tid; k < sum; k += kScopeOpsBlock)
        if (base + k < out_cap) out[base + k] = sA[k];
}

// out[i] = first + i, one store per thread.  The blocks are laid out in two grid dimensions: a launch may hold fewer than
// 2^32 threads per dimension, and a range of 2^32 - 1 ids needs 2^24 blocks of 256.
constexpr uint32_t kScopeRangeGridX = 1u << 20;

__global__ void __launch_bounds__(kScopeOpsBlock)
scope_range_kernel(uint32_t first, uint64_t n, uint32_t* __restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.y * gridDim.x + blockIdx.x) * kScopeOpsBlock + threadIdx.x;
    if (i < n) out[i] = first + (uint32_t)i;
}

int32_t launch_scope_ops_count(const uint32_t* d_a, uint64_t na, const uint32_t* d_b, uint64_t nb, int32_t op, uint32_t* d_tiles,
                               hipStream_t stream) {
    const uint32_t nt = (uint32_t)scope_ops_tiles(na, nb);
    if (nt == 0) {
        CS_HIP(hipMemsetAsync(d_tiles, 0, sizeof(uint32_t), stream));
        return CS_OK;
    }
    hipLaunchKernelGGL(scope_ops_kernel<false>, dim3(nt), dim3(kScopeOpsBlock), 0, stream, d_a, na, d_b, nb, op, d_tiles,
                       (uint32_t*)nullptr, (uint64_t)0);
    CS_HIP(hipGetLastError());
    return launch_mask_scan(d_tiles, nt, stream);
}

int32_t launch_scope_ops_write(const uint32_t* d_a, uint64_t na, const uint32_t* d_b, uint64_t nb, int32_t op, uint32_t* d_tiles,
                               uint32_t* d_out, uint64_t out_cap, hipStream_t stream) {
    const uint32_t nt = (uint32_t)scope_ops_tiles(na, nb);
    if (nt == 0 || out_cap == 0) return CS_OK;
    hipLaunchKernelGGL(scope_ops_kernel<true>, dim3(nt), dim3(kScopeOpsBlock), 0, stream, d_a, na, d_b, nb, op, d_tiles, d_out,
                       out_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_scope_range(uint32_t first, uint64_t n, uint32_t* d_out, hipStream_t stream) {
    if (n == 0) return CS_OK;
    const uint64_t blocks = (n + kScopeOpsBlock - 1) / kScopeOpsBlock;  // <= 2^24: n < 2^32
    const uint32_t gx = blocks < kScopeRangeGridX ? (uint32_t)blocks : kScopeRangeGridX;
    hipLaunchKernelGGL(scope_range_kernel, dim3(gx, (uint32_t)((blocks + gx - 1) / gx)), dim3(kScopeOpsBlock), 0, stream, first, n,
                       d_out);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
