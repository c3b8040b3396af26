// scan_clusters_scoped.hip — the scoped similar-clusters search (cs_index_similar_clusters_scoped): the clone classes
// inside one scope or between two, i.e. the connected components of the graph whose vertices are the live ids of A u B and
// whose edges are the pairs cs_index_similar_pairs_scoped would count.  Plan: clusters_scoped_plan.hpp.
//
//   pack     launch_pairs_pack of scan_pairs_scoped.hip, unchanged: list entry i of a scope -> packed row i of an f16 buffer
//            of the call's own, with the bits the index's own copy holds for that row (the margin argument rests on that).
//   init     cscoped_init_kernel: parent[r] = r, mark[r] = 0 for the rows of the lists, and for no other word.
//   join     cscoped_join_kernel: pairs_scoped_filter_kernel's operand side (scan_pairs_scoped.hip: two packed bases and two
//            row maps, a runtime triangle / rectangle flag with the diagonal tile staged once, 128 x 128 x dim on
//            v_mfma_f32_32x32x16_f16, two LDS-DMA stages of 16 KiB, the LDS image and swizzle of uf_mainloop, the k-walk
//            rotated per block, 256 threads, two blocks per CU) under clusters_join_kernel's epilogue (scan_clusters.hip:
//            three classes against min_cos -+ margin, the norm-range proviso for "certain", the two-pass mask form, one
//            wave-level atomic per round for the ambiguous appends, the early over / same-root exit taken by one thread) —
//            both restated here so that those files' text, and with it their device code, stays what it is.
//   rescore  launch_clusters_rescore of scan_clusters.hip, unchanged: the ambiguous pairs are STORED rows (lower | higher
//            << 32 through the lists), so the cosine bits are the unscoped call's by construction.
//   roots    cscoped_tile_root_kernel, between launches: one array per side over PACKED tiles through the list.  No packed
//            tile is empty (the lists hold live rows only, and a side of n rows has ceil(n / 128) tiles).
//   label    cscoped_label_kernel over the lists: flatten, write (id, label id) per list entry, count classes and members.
//
// THE UNION-FIND STAYS OVER STORED ROWS.  parent[] and mark[] are indexed by stored row and sized by stored rows, but only
// the words of the scopes' rows are initialised, and every kernel after that reaches only those words: a find starts at a
// row of a list and follows parents, and a parent is only ever set (init, hook, halving) to a row of a list.  So the device
// work and traffic of a call are O(live rows of the scopes), not O(stored rows), and every invariant of scan_clusters.hip's
// header carries over word for word: a hook is ONE agent-scope atomicCAS(&parent[hi], hi, lo) with lo < hi, so parent[r] <=
// r always, chains strictly descend, a root is the smallest row of its tree and a row that stopped being a root never is
// one again; a lost CAS goes on from the value it returned; path halving stores an ancestor into a NON-root's word, and no
// CAS expects a non-root, so the two never collide; reads are agent-scope relaxed atomic loads and a stale read is
// harmless.  Rows ascend with ids, also after a reclaiming build (index_ledger.hpp), so the label — the root's id — is the
// smallest id of the component, with no vertex renumbering.  A row that sits in both lists is one vertex by construction.
//
// WHAT IS DROPPED relative to the scoped filter.  The duplicate rule and its binary searches: uniting is idempotent, so
// the rectangle visiting a pair of A n B twice is harmless; only a hit whose two stored rows are EQUAL is dropped (a row is
// no pair with itself).  The tombstone test: the lists hold live rows only, and packed rows past a list's end are masked.
// "CERTAIN" is scan_clusters.hip's argument unchanged: the packed rows carry the index's own f16 bits, so filter_margin(dim)
// bounds |f16 product - exact cosine| wherever the rows sit, and the shortcut is taken only for two rows whose stored
// norms both lie in (1e-15, 1e15).
#include "clusters_scoped_plan.hpp"
#include "grouped_plan.hpp"  // kNoGroup
#include "scan.hpp"
#include "split_f16.hpp"

namespace cs {

namespace {

// Offset (in f16 elements) of (row, k-chunk c) in the tiled filter layout — uf_tiled_off of scan_filter.hip.
__device__ __forceinline__ size_t cscoped_tiled_off(uint64_t row, uint32_t c, uint32_t kchunks) {
    return (((row >> 7) * kchunks + c) * 128 + (row & 127)) * 64;
}

// The group of an id as every kernel reads the table (scan_similar.hip similar_group_of): ids past its end are ungrouped.
__device__ __forceinline__ uint32_t cscoped_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

// ---- the union-find of scan_clusters.hip, restated (its header holds the proof) ----
__device__ __forceinline__ uint32_t cscoped_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way (any ancestor may be stored).
__device__ __forceinline__ uint32_t cscoped_find(uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = cscoped_load(parent + x);
    while (p != x) {
        const uint32_t g = cscoped_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// The root of x without a store (the label kernel reads a forest nobody hooks any more).
__device__ __forceinline__ uint32_t cscoped_root(const uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = cscoped_load(parent + x);
    while (p != x) {
        x = p;
        p = cscoped_load(parent + x);
    }
    return x;
}

// Hooks the larger root under the smaller.  Lock-free: a lost CAS goes on from the value it returned.
__device__ __forceinline__ void cscoped_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cscoped_find(parent, a);
        b = cscoped_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;  // hi got a parent meanwhile: an ancestor of hi, below it
        b = lo;
    }
}

// Entry i of the two lists laid end to end (B's after A's; nB == 0: one list).  A row in both is written twice, the same
// values both times.
__global__ void __launch_bounds__(256)
cscoped_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ mark, const uint32_t* __restrict__ listA, uint64_t nA,
                    const uint32_t* __restrict__ listB, uint64_t nB) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (uint64_t)gridDim.x * 256) {
        const uint32_t r = i < nA ? listA[i] : listB[i - nA];
        parent[r] = r;
        mark[r] = 0u;
    }
}

// grid = the side's packed tiles, 128 threads: one packed row each.
__global__ void __launch_bounds__(128)
cscoped_tile_root_kernel(uint32_t* __restrict__ parent, const uint32_t* __restrict__ list, uint64_t n_list,
                         uint32_t* __restrict__ tile_root) {
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0u; }
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    if (p < n_list) {
        const uint32_t r = cscoped_find(parent, list[p]);
        atomicMin(&s_min, r);
        atomicMax(&s_max, r);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        tile_root[blockIdx.x] = s_min == 0xFFFFFFFFu ? kClustersEmptyTile : (s_min == s_max ? s_min : kClustersNoRoot);
}

// grid = PairsPlan::band_blocks(band_count), dynamic LDS = SH_LDS_BYTES; the block -> tile pair map of
// pairs_scoped_filter_kernel.  tri: baseB == baseA, listB == listA, nB == nA, rootB == rootA, tiles = the side's packed
// tiles; else tiles = the B side's.  counters[0] = ambiguous pairs counted (past `cap`: the launch is void and its range is
// split), [1] = tile pairs skipped.
__global__ void __launch_bounds__(256, 2)
cscoped_join_kernel(const _Float16* __restrict__ baseA, const _Float16* __restrict__ baseB, const uint32_t* __restrict__ listA,
                    const uint32_t* __restrict__ listB, uint32_t nA, uint32_t nB, uint32_t kchunks, int tri, uint64_t tiles,
                    uint64_t band_first, uint64_t band_count, uint64_t xcd_run, RowIds ids, GroupView gv, int other_group,
                    float lo, float hi, const float* __restrict__ norms, uint32_t* __restrict__ parent,
                    const uint32_t* __restrict__ rootA, const uint32_t* __restrict__ rootB, uint64_t* __restrict__ amb,
                    unsigned long long* __restrict__ counters, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint64_t in_band = (uint64_t)(blockIdx.x & 7) * xcd_run + (blockIdx.x >> 3);
    if (in_band >= band_count) return;
    uint64_t ti, tj;
    if (tri) tile_pair_of(band_first + in_band, tiles, ti, tj);
    else rect_pair_of(band_first + in_band, tiles, ti, tj);
    // ONE thread takes the block's decision (barriers follow): the buffer is already over — this launch is void whatever
    // the block finds — or the two tiles are already one component
    if (threadIdx.x == 0) {
        // (the three loads are independent and issued together: one memory latency in front of the block, not two)
        const uint32_t ra = rootA[ti], rb = rootB[tj];
        const bool over = __hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap;
        const bool same = ra == kClustersEmptyTile || rb == kClustersEmptyTile || (ra == rb && ra != kClustersNoRoot);
        if (same && !over) atomicAdd(counters + 1, 1ull);
        *reinterpret_cast<volatile uint32_t*>(lds) = (over || same) ? 1u : 0u;
    }
    __syncthreads();
    const bool skip = *reinterpret_cast<volatile uint32_t*>(lds) != 0;
    __syncthreads();  // the word is read before the first stage overwrites it
    if (skip) return;
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
            // every packed tile is whole in its buffer: rows past the list's end are zeros, and masked in the epilogue
            asrc[i] = baseA + cscoped_tiled_off(ti * 128 + row, 0, kchunks) + c * 8;
            wsrc[i] = baseB + cscoped_tiled_off(tj * 128 + row, 0, kchunks) + c * 8;
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

    // not ruled out <=> product > min_cos - margin, written so that NaN counts.  Almost every wave holds none.
    unsigned long long any = 0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) any |= __ballot(!(acc[i][j][r] <= lo));
    if (!any) return;

    // Pass 1, unrolled over the accumulator: per lane one bit per element that passed every test (bit (2 j + i) 16 + r) and
    // one that says "certain".  Pass 2 walks the bits, not the accumulator — the union loop below is unbounded, and an
    // unrolled loop around it would be kept rolled and take the accumulator out of its registers.
    unsigned long long hits = 0, sures = 0;
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
                const float v = acc[i][j][r];
                bool hit = !(v <= lo) && pB < nB && pA < nA && (!diag || m < n);
                if (!__ballot(hit)) continue;  // wave-uniform
                uint32_t rA = 0, rB = 0;
                if (hit) {  // the maps are read below the lists' lengths only
                    rA = listA[pA];
                    rB = listB[pB];
                    hit = rA != rB;  // (rectangle: a row of both lists met itself)
                }
                if (hit && other_group) {  // two group reads per hit; two ungrouped chunks are never one file
                    const uint32_t ga = cscoped_group_of(gv, ids.of(rA)), gb = cscoped_group_of(gv, ids.of(rB));
                    hit = !(ga == gb && ga != kNoGroup);
                }
                // certain: above the upper bound, finite, and both rows of ordinary magnitude (the header)
                bool sure = hit && v > hi && v < __builtin_huge_valf();
                if (sure) {
                    const float na = norms[rA], nb = norms[rB];
                    sure = na > 1e-15f && na < 1e15f && nb > 1e-15f && nb < 1e15f;
                }
                const unsigned long long bit = 1ull << ((2 * j + i) * 16 + r);
                if (hit) hits |= bit;
                if (sure) sures |= bit;
            }
        }
    }
    // Pass 2: every lane takes its lowest bit per round — a certain pair is united here, the others of the round are
    // appended with ONE atomic for the wave (one atomic per lane on one address serialises at the L2).
    while (__ballot(hits != 0)) {  // wave-uniform
        const bool have = hits != 0;
        const int bit = have ? __ffsll((long long)hits) - 1 : 0;
        const bool sure = have && ((sures >> bit) & 1ull);
        hits &= hits - 1;  // (0 stays 0)
        const int r = bit & 15, i = (bit >> 4) & 1, j = bit >> 5;
        uint32_t rA = 0, rB = 0;
        if (have) {  // a bit is set only below the lists' lengths
            rA = listA[ti * 128 + (uint32_t)(wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h)];
            rB = listB[tj * 128 + (uint32_t)(wc * 64 + j * 32 + l31)];
        }
        if (sure) cscoped_unite(parent, rA, rB);
        const bool open = have && !sure;
        const unsigned long long mask = __ballot(open);
        if (!mask) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(counters, (unsigned long long)__popcll(mask));  // keeps counting past cap; stores stop at it
        base = __shfl(base, 0, 64);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (open && base + before < cap) {
            const uint64_t lower = rA < rB ? rA : rB, higher = rA < rB ? rB : rA;
            amb[base + before] = lower | (higher << 32);
        }
    }
}

// Entry i of the two lists laid end to end -> out_ids[i] = its id, out_label[i] = the id of its row's root.  mark[r]: bit 0
// "this root's class was counted", bit 1 "this row was counted as a member" — a row in both lists is met twice and counted
// once, a root is counted once however many members reach it.  totals[0] = classes of two or more, totals[1] = ids in
// them: sums of integers, the same whatever the order.
__global__ void __launch_bounds__(256)
cscoped_label_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ mark, const uint32_t* __restrict__ listA, uint64_t nA,
                     const uint32_t* __restrict__ listB, uint64_t nB, RowIds ids, uint32_t* __restrict__ out_ids,
                     uint32_t* __restrict__ out_label, unsigned long long* __restrict__ totals) {
    __shared__ uint32_t s_clusters, s_members;
    if (threadIdx.x == 0) { s_clusters = 0u; s_members = 0u; }
    __syncthreads();
    uint32_t clusters = 0, members = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nA + nB; i += (uint64_t)gridDim.x * 256) {
        const uint32_t r = i < nA ? listA[i] : listB[i - nA];
        const uint32_t root = cscoped_root(parent, r);
        // flatten: the root is an ancestor, and other threads' walks through this word stay walks to the same root
        if (root != r) __hip_atomic_store(parent + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        out_ids[i] = ids.of(r);
        out_label[i] = ids.of(root);
        if (root != r && (atomicOr(mark + r, 2u) & 2u) == 0u) {
            ++members;
            if ((atomicOr(mark + root, 1u) & 1u) == 0u) { ++clusters; ++members; }
        }
    }
    if (clusters) atomicAdd(&s_clusters, clusters);
    if (members) atomicAdd(&s_members, members);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_clusters) atomicAdd(totals, (unsigned long long)s_clusters);
        if (s_members) atomicAdd(totals + 1, (unsigned long long)s_members);
    }
}

uint32_t cscoped_entry_blocks(uint64_t n) {
    const uint64_t want = (n + 255) / 256;
    return (uint32_t)(want < 1 ? 1 : (want > 65536 ? 65536 : want));
}

}  // namespace

int32_t launch_clusters_scoped_init(uint32_t* d_parent, uint32_t* d_mark, const uint32_t* d_list_a, uint64_t rows_a,
                                    const uint32_t* d_list_b, uint64_t rows_b, hipStream_t stream) {
    if (rows_a + rows_b == 0) return CS_OK;
    hipLaunchKernelGGL(cscoped_init_kernel, dim3(cscoped_entry_blocks(rows_a + rows_b)), dim3(256), 0, stream, d_parent, d_mark,
                       d_list_a, rows_a, d_list_b, rows_b);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_scoped_tile_roots(uint32_t* d_parent, const uint32_t* d_list, uint64_t rows, uint32_t* d_tile_root,
                                          hipStream_t stream) {
    const uint64_t tiles = packed_tiles_of(rows);
    if (tiles == 0) return CS_OK;
    if (tiles > 0x7FFFFFFFull)
        return fail(CS_ERR_BAD_ARG, "scoped similar-clusters tile roots: %llu packed tiles", (unsigned long long)tiles);
    hipLaunchKernelGGL(cscoped_tile_root_kernel, dim3((uint32_t)tiles), dim3(128), 0, stream, d_parent, d_list, rows, d_tile_root);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_scoped_join(const ClustersScopedPlan& plan, const _Float16* d_packed_a, const _Float16* d_packed_b,
                                    const uint32_t* d_list_a, const uint32_t* d_list_b, uint32_t dim, uint64_t first,
                                    uint64_t count, RowIds ids, const GroupView& gv, bool other_group, float min_cos,
                                    float margin, const float* d_norms, uint32_t* d_parent, const uint32_t* d_root_a,
                                    const uint32_t* d_root_b, uint64_t* d_amb, uint64_t* d_counters, hipStream_t stream) {
    if (!split_scan_supported(dim))
        return fail(CS_ERR_UNSUPPORTED, "scoped similar-clusters join: dim must be 384, 768 or 1024, got %u", dim);
    if (count == 0) return CS_OK;
    if (count > kPairsBandTilePairs || first + count > plan.tile_pairs || plan.rows_a > 0xffffffffull ||
        plan.rows_b > 0xffffffffull || plan.tiles_a != packed_tiles_of(plan.rows_a) || plan.tiles_b != packed_tiles_of(plan.rows_b) ||
        plan.tile_pairs != (plan.triangle ? tile_pairs_of(plan.tiles_a) : plan.tiles_a * plan.tiles_b) ||
        plan.ambiguous_cap < kClustersAmbiguousMin || plan.ambiguous_cap > 0xffffffffull || !d_norms ||
        (plan.triangle && (d_packed_a != d_packed_b || d_list_a != d_list_b || d_root_a != d_root_b || plan.rows_a != plan.rows_b)))
        return fail(CS_ERR_BAD_ARG, "scoped similar-clusters join: launch [%llu, +%llu) outside the %s of %llu x %llu tiles",
                    (unsigned long long)first, (unsigned long long)count, plan.triangle ? "triangle" : "rectangle",
                    (unsigned long long)plan.tiles_a, (unsigned long long)plan.tiles_b);
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&cscoped_join_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   SH_LDS_BYTES));
        return CS_OK;
    }));
    const uint64_t run = PairsPlan::xcd_run(count);
    hipLaunchKernelGGL(cscoped_join_kernel, dim3((uint32_t)PairsPlan::band_blocks(count)), dim3(256), SH_LDS_BYTES, stream,
                       d_packed_a, d_packed_b, d_list_a, d_list_b, (uint32_t)plan.rows_a, (uint32_t)plan.rows_b, dim / 64,
                       plan.triangle ? 1 : 0, plan.triangle ? plan.tiles_a : plan.tiles_b, first, count, run, ids, gv,
                       other_group ? 1 : 0, min_cos - margin, min_cos + margin, d_norms, d_parent, d_root_a, d_root_b, d_amb,
                       reinterpret_cast<unsigned long long*>(d_counters), (uint32_t)plan.ambiguous_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_scoped_label(uint32_t* d_parent, uint32_t* d_mark, const uint32_t* d_list_a, uint64_t rows_a,
                                     const uint32_t* d_list_b, uint64_t rows_b, RowIds ids, uint32_t* d_out_ids,
                                     uint32_t* d_out_label, uint64_t* d_totals, hipStream_t stream) {
    if (rows_a + rows_b == 0) return CS_OK;
    hipLaunchKernelGGL(cscoped_label_kernel, dim3(cscoped_entry_blocks(rows_a + rows_b)), dim3(256), 0, stream, d_parent, d_mark,
                       d_list_a, rows_a, d_list_b, rows_b, ids, d_out_ids, d_out_label,
                       reinterpret_cast<unsigned long long*>(d_totals));
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
