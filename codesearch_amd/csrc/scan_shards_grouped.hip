// scan_shards_grouped.hip — the root's capped shard merge of a grouped search over a sharded store (shards.hip
// cs_shards_search_grouped*).  Host plan, levels and why no new lemma is needed: shards_grouped_plan.hpp.
//
// Every shard leaves its capped best k per query in the root's gather buffer as (cosine, LOCAL row) keys, zeros behind the
// count: list s of query q at in + (s * nq + q) * k.  A shard caps under its own table, so a group spread over N shards can
// still hold N * per_group slots here: this level caps again, under the root's table by GLOBAL id.
// A kernel of its own file: the kernels of scan_grouped.hip stay, byte for byte, what they were
// (benchmarks/compare_device_code.py; profiles/shards_grouped_device_code.log).
#include "scan.hpp"
#include "shards_grouped_plan.hpp"
#include "scan_wave.hpp"
#include "scan_rules.hpp"

namespace cs {

// Block (g, q) takes shards [g * G, min(N, (g + 1) * G)) of query q and writes its capped best k, as GLOBAL keys, to
// out_keys[q][g][k], best first, zeros behind; with one block per query that is the answer.  Per block:
//   the keys are read and every local row becomes its global id (shards_global_of: monotone inside a shard, so a shard's
//   order is its global order);
//   from there it is merge_topk_grouped_kernel (scan_grouped.hip), step for step: a[] = the keys, sorted; b[] =
//   (group << 32 | ~position) images of the non-empty keys, the group read from the root's table, sorted; a key whose image
//   per_group places earlier has the same group is zeroed (never for kNoGroup); ordered compaction, the first k leave.
// LDS: 2 * nsort * 8 B, at most 64 KB (opt-in per device, as there).  1,024 threads: the kernel runs once per query on a
// root stream that has nothing else to do, and the sort's barriers are what it waits for.
constexpr int kSGMergeBlock = 1024;
constexpr int kSGMergePer = kGroupedMergeCap / kSGMergeBlock;

__global__ void __launch_bounds__(kSGMergeBlock)
merge_shards_grouped_kernel(const uint64_t* __restrict__ in, uint32_t nshards, uint32_t nq, uint32_t k, uint32_t G,
                            uint32_t stripe, GroupView gv, uint64_t* __restrict__ out_keys) {
    extern __shared__ __attribute__((aligned(16))) uint64_t a[];  // [nsort] keys, [nsort] images
    __shared__ uint32_t wave_tot[kSGMergeBlock / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t g = blockIdx.x, q = blockIdx.y, ngroups = gridDim.x;
    const uint32_t lo = g * G;
    const uint32_t hi = (lo + G < nshards) ? lo + G : nshards;
    const uint32_t ncand = (hi - lo) * k;  // <= kGroupedMergeCap (the launcher's G)
    uint32_t nsort = 64;
    while (nsort < ncand) nsort <<= 1;
    uint64_t* const b = a + nsort;
    for (uint32_t i = tid; i < nsort; i += kSGMergeBlock) {
        uint64_t key = 0ull;
        if (i < ncand) {
            const uint32_t l = i / k, e = i - l * k;
            key = in[((size_t)(lo + l) * nq + q) * k + e];
            if (key) key = (key & 0xffffffff00000000ull) | (uint64_t)(~shards_global_of(key_id(key), stripe, nshards, lo + l));
        }
        a[i] = key;
    }
    block_bitonic_desc<kSGMergeBlock>(a, nsort, tid);
    for (uint32_t i = tid; i < nsort; i += kSGMergeBlock) {
        const uint64_t key = a[i];
        b[i] = key ? (((uint64_t)group_of(gv, key_id(key)) << 32) | (uint64_t)(0xffffffffu - i)) : 0ull;
    }
    block_bitonic_desc<kSGMergeBlock>(b, nsort, tid);
    const uint32_t m = gv.per_group;
    for (uint32_t i = tid; i < nsort; i += kSGMergeBlock) {
        const uint64_t v = b[i];
        const uint32_t grp = (uint32_t)(v >> 32);
        // images before a non-empty one are non-empty (empty = 0 sorts last)
        if (v && grp != kNoGroup && i >= m && (uint32_t)(b[i - m] >> 32) == grp) a[0xffffffffu - (uint32_t)v] = 0ull;
    }
    __syncthreads();
    // ordered compaction: thread t owns a[t * kSGMergePer, +kSGMergePer)
    uint64_t mine[kSGMergePer];
    uint32_t cnt = 0;
#pragma unroll
    for (int j = 0; j < kSGMergePer; ++j) {
        const uint32_t i = (uint32_t)tid * kSGMergePer + j;
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
    for (int w = 0; w < kSGMergeBlock / 64; ++w) {
        pos += (w < wave) ? wave_tot[w] : 0u;
        total += wave_tot[w];
    }
    const uint32_t kept = total < k ? total : k;
    uint64_t* const okeys = out_keys + ((size_t)q * ngroups + g) * k;
#pragma unroll
    for (int j = 0; j < kSGMergePer; ++j) {
        if (mine[j] == 0ull) continue;
        if (pos < k) okeys[pos] = mine[j];
        ++pos;
    }
    for (uint32_t i = kept + tid; i < k; i += kSGMergeBlock) okeys[i] = 0ull;  // the slots no survivor fills
}

// ---- host side ------------------------------------------------------------------------------------------

int32_t launch_merge_shards_grouped(const ShardsGroupedPlan& plan, const uint64_t* d_gathered, uint32_t nshards, uint32_t nq,
                                    uint32_t k, uint32_t stripe, const GroupView& gv, uint64_t* d_first, uint64_t* d_tmp_a,
                                    uint64_t* d_tmp_b, uint64_t* d_out_keys, hipStream_t stream) {
    if (gv.per_group == 0) return fail(CS_ERR_BAD_ARG, "per_group must be at least 1");
    const uint32_t G = plan.group;
    if (!d_gathered || !d_out_keys || nshards == 0 || nq == 0 || k == 0 || stripe == 0 || G == 0 ||
        (uint64_t)G * k > kGroupedMergeCap || plan.first_lists != (nshards + G - 1) / G)
        return fail(CS_ERR_BAD_ARG, "grouped shard merge takes at most %u keys per block", kGroupedMergeCap);
    const bool final_pass = plan.first_lists == 1;
    if (!final_pass && !d_first) return fail(CS_ERR_BAD_ARG, "merge scratch missing");
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(merge_shards_grouped_kernel),
                                   hipFuncAttributeMaxDynamicSharedMemorySize, 2 * kGroupedMergeCap * sizeof(uint64_t)));
        return CS_OK;
    }));
    const uint32_t take = nshards < G ? nshards : G;
    uint32_t nsort = 64;
    while (nsort < take * k) nsort <<= 1;
    hipLaunchKernelGGL(merge_shards_grouped_kernel, dim3(plan.first_lists, nq), dim3(kSGMergeBlock),
                       (size_t)2 * nsort * sizeof(uint64_t), stream, d_gathered, nshards, nq, k, G, stripe, gv,
                       final_pass ? d_out_keys : d_first);
    CS_HIP(hipGetLastError());
    if (final_pass) return CS_OK;
    // ids are global from here on: the ordinary capped merge under the same table, every level capping
    return launch_merge_grouped(plan.rest, d_first, nq, k, gv, d_tmp_a, d_tmp_b, d_out_keys, nullptr, nullptr, nullptr, stream);
}

}  // namespace cs
