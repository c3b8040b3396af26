// scan_clusters.hip — the similar-clusters search (cs_index_similar_clusters): the clone classes of the store, i.e. the
// connected components of the graph whose edges are the pairs cs_index_similar_pairs would count.  The answer is one label
// per id, so nothing here grows with the number of pairs.
//
//   join     clusters_join_kernel: pairs_filter_kernel's tile product (scan_pairs.hip: one block per pair of 128-row tiles
//            ti <= tj of the tiled f16 unit copy, 128 x 128 x dim on v_mfma_f32_32x32x16_f16, both operands brought in by
//            LDS-DMA in 16-KiB stages with the staging, LDS image and swizzle of uf_mainloop, the k-walk rotated per block,
//            on the diagonal one staged tile and only rowA < rowB) — its text restated here so that scan_pairs.hip, and
//            with it its device code, stays what it is.  The epilogue sorts every element into one of three classes:
//              acc <= min_cos - margin              no edge (the pairs call's own test);
//              acc >  min_cos + margin, finite      an edge FOR CERTAIN (below): united straight from the epilogue;
//              anything else, NaN included          AMBIGUOUS: parked as (rowA | rowB << 32) in the ambiguous buffer;
//            the last two after the stored-row, tombstone and group tests of the pairs call.
//   rescore  clusters_rescore_kernel: every ambiguous pair re-scored from the f32 corpus with pairs_rescore_kernel's
//            layout and operation order (the similar scan's bits, the lower id's row as the query) and united only if the
//            cosine is finite and strictly above min_cos.
//   roots    clusters_tile_root_kernel, between launches: tile_root[t] = the common root of tile t's live rows, or none.  A
//            join block whose two tiles carry the same root returns after that one comparison.
//   label    clusters_label_kernel: parent flattened, labels written as ids, clusters and members counted.
//
// THE UNION-FIND.  parent[stored_rows] (u32, HBM), parent[r] = r at the start.  A hook is ONE agent-scope
// atomicCAS(&parent[hi], hi, lo) with lo < hi, both roots as its caller last saw them; so parent[r] <= r always, a chain
// of parents strictly descends (finds end), a root is the smallest row of its tree, and a row that stopped being a root
// never is one again.  A lost CAS returns the parent that hi got meanwhile and the caller goes on from it: no wave ever
// waits for another, and every failure is somebody else's success, of which there are fewer than stored_rows.  Path
// halving stores an ancestor of x into parent[x] for a non-root x: whatever interleaving, the value stays an ancestor
// (ancestry is never undone), and no CAS expects a non-root, so halving and hooking never collide on a word.  Reads are
// agent-scope relaxed atomic loads: the L2s are per XCD, and a plain load may be served from a line another XCD has since
// changed.  A STALE read is still harmless — a former parent is an ancestor, a former root fails its CAS — so no ordering
// between different words is needed; the kernel boundary publishes everything to the next launch.
// The components do not depend on the order of the hooks, and each root is its component's smallest row; rows ascend
// with ids (index_ledger.hpp: a reclaim keeps the survivors in order), so the label is the smallest id.
//
// WHY "acc > min_cos + margin" IS CERTAIN.  filter_margin(dim) is a two-sided bound on |f16 product - exact cosine| of the
// unit rows (scan_filter.hip's header), with 2e-5 of slack for the f32 rounding of the unit rows.  The unit rows' rounding
// uses under 6e-6 of it (x / |x|: one division, and a norm whose relative error is a few dozen ulp: < 3e-6 a side at dim
// 1024), and the similar scan's own cosine — chains of dim / 32 fmaf, five butterfly adds, two square roots, a product and
// a division — is within 5e-6 of the exact one WHEN NOTHING OVER- OR UNDERFLOWS; together under 1.1e-5.  So acc > min_cos +
// margin puts the scan's cosine above min_cos by at least 9e-6: it qualifies, finite, whatever its last bits are — and the
// answer carries no cosine.  The proviso is checked, not assumed: the shortcut is taken only for two rows whose stored
// norms both lie in (1e-15, 1e15), where sums of squares and dot products stay in f32's normal range; every other pair
// above the lower bound is ambiguous and the rescore decides it with the scan's own arithmetic.
#include "clusters_plan.hpp"
#include "grouped_plan.hpp"  // kNoGroup
#include "scan.hpp"
#include "split_f16.hpp"

namespace cs {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Offset (in f16 elements) of (row, k-chunk c) in the tiled filter copy — uf_tiled_off of scan_filter.hip.
__device__ __forceinline__ size_t clusters_tiled_off(uint64_t row, uint32_t c, uint32_t kchunks) {
    return (((row >> 7) * kchunks + c) * 128 + (row & 127)) * 64;
}

// The group of an id as every kernel reads the table (scan_similar.hip similar_group_of): ids past its end are ungrouped.
__device__ __forceinline__ uint32_t clusters_group_of(const GroupView& gv, uint32_t id) {
    const uint32_t i = id - gv.id_base;
    return (gv.groups && i < gv.len) ? gv.groups[i] : kNoGroup;
}

__device__ __forceinline__ uint32_t uf_load(const uint32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x, halving the path on the way (any ancestor may be stored: the header).
__device__ __forceinline__ uint32_t uf_find(uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = uf_load(parent + x);
    while (p != x) {
        const uint32_t g = uf_load(parent + p);
        if (g != p) __hip_atomic_store(parent + x, g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        x = p;
        p = g;
    }
    return x;
}

// The root of x without a store (the label kernel reads a forest nobody changes any more).
__device__ __forceinline__ uint32_t uf_root(const uint32_t* __restrict__ parent, uint32_t x) {
    uint32_t p = uf_load(parent + x);
    while (p != x) {
        x = p;
        p = uf_load(parent + x);
    }
    return x;
}

// Hooks the larger root under the smaller.  Lock-free: a lost CAS goes on from the value it returned.
__device__ __forceinline__ void uf_unite(uint32_t* __restrict__ parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;  // hi got a parent meanwhile: an ancestor of hi, below it
        b = lo;
    }
}

__global__ void __launch_bounds__(256)
clusters_init_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ mark, uint64_t n_rows) {
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256) {
        parent[r] = (uint32_t)r;
        mark[r] = 0u;
    }
}

// grid = tiles, 128 threads: one row each.
__global__ void __launch_bounds__(128)
clusters_tile_root_kernel(uint32_t* __restrict__ parent, uint64_t n_rows, const uint32_t* __restrict__ dead,
                          uint32_t* __restrict__ tile_root) {
    __shared__ uint32_t s_min, s_max;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_max = 0u; }
    __syncthreads();
    const uint64_t row = (uint64_t)blockIdx.x * 128 + threadIdx.x;
    bool live = row < n_rows;
    if (live && dead) live = !((dead[row >> 5] >> (row & 31)) & 1u);
    if (live) {
        const uint32_t r = uf_find(parent, (uint32_t)row);
        atomicMin(&s_min, r);
        atomicMax(&s_max, r);
    }
    __syncthreads();
    if (threadIdx.x == 0)
        tile_root[blockIdx.x] = s_min == 0xFFFFFFFFu ? kClustersEmptyTile : (s_min == s_max ? s_min : kClustersNoRoot);
}

// grid = PairsPlan::band_blocks(count), dynamic LDS = SH_LDS_BYTES; the block -> tile pair map of pairs_filter_kernel.
// counters[0] = ambiguous pairs counted (past `cap`: the launch is void and its range is split), [1] = tile pairs skipped.
__global__ void __launch_bounds__(256, 2)
clusters_join_kernel(const _Float16* __restrict__ corpus_h, uint32_t kchunks, uint64_t tiles, uint64_t band_first,
                     uint64_t band_count, uint64_t xcd_run, uint64_t n_rows, const uint32_t* __restrict__ dead, RowIds ids,
                     GroupView gv, int other_group, float lo, float hi, const float* __restrict__ norms,
                     uint32_t* __restrict__ parent, const uint32_t* __restrict__ tile_root, uint64_t* __restrict__ amb,
                     unsigned long long* __restrict__ counters, uint32_t cap) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint64_t in_band = (uint64_t)(blockIdx.x & 7) * xcd_run + (blockIdx.x >> 3);
    if (in_band >= band_count) return;
    uint64_t ti, tj;
    tile_pair_of(band_first + in_band, tiles, ti, tj);
    // ONE thread takes the block's decision (barriers follow): the buffer is already over — this launch is void whatever
    // the block finds — or the two tiles are already one component (or one of them holds no live row)
    if (threadIdx.x == 0) {
        // (the three loads are independent and issued together: one memory latency in front of the block, not two)
        const uint32_t ra = tile_root[ti], rb = tile_root[tj];
        const bool over = __hip_atomic_load(counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > cap;
        const bool same = ra == kClustersEmptyTile || rb == kClustersEmptyTile || (ra == rb && ra != kClustersNoRoot);
        if (same && !over) atomicAdd(counters + 1, 1ull);
        *reinterpret_cast<volatile uint32_t*>(lds) = (over || same) ? 1u : 0u;
    }
    __syncthreads();
    const bool skip = *reinterpret_cast<volatile uint32_t*>(lds) != 0;
    __syncthreads();  // the word is read before the first stage overwrites it
    if (skip) return;
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
            // rows past n_rows exist in the copy's padded last tile; they are masked in the epilogue
            asrc[i] = corpus_h + clusters_tiled_off(ti * 128 + row, 0, kchunks) + c * 8;
            wsrc[i] = corpus_h + clusters_tiled_off(tj * 128 + row, 0, kchunks) + c * 8;
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
        const uint64_t rowB = tj * 128 + n;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t m = wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                const uint64_t rowA = ti * 128 + m;
                const float v = acc[i][j][r];
                bool hit = !(v <= lo) && rowB < n_rows && rowA < n_rows && (!diag || m < n);
                if (!__ballot(hit)) continue;  // wave-uniform
                if (hit && dead) hit = !(((dead[rowA >> 5] >> (rowA & 31)) | (dead[rowB >> 5] >> (rowB & 31))) & 1u);
                if (hit && other_group) {  // two group reads per hit; two ungrouped chunks are never one file
                    const uint32_t ga = clusters_group_of(gv, ids.of(rowA)), gb = clusters_group_of(gv, ids.of(rowB));
                    hit = !(ga == gb && ga != kNoGroup);
                }
                // certain: above the upper bound, finite, and both rows of ordinary magnitude (the header)
                bool sure = hit && norms != nullptr && v > hi && v < __builtin_huge_valf();
                if (sure) {
                    const float na = norms[rowA], nb = norms[rowB];
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
        const uint64_t rowA = ti * 128 + (uint32_t)(wr * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * h);
        const uint64_t rowB = tj * 128 + (uint32_t)(wc * 64 + j * 32 + l31);
        if (sure) uf_unite(parent, (uint32_t)rowA, (uint32_t)rowB);
        const bool open = have && !sure;
        const unsigned long long mask = __ballot(open);
        if (!mask) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(counters, (unsigned long long)__popcll(mask));  // keeps counting past cap; stores stop at it
        base = __shfl(base, 0, 64);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        if (open && base + before < cap) amb[base + before] = rowA | (rowB << 32);
    }
}

__device__ __forceinline__ float clusters_half_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 8, 64);
    v += __shfl_xor(v, 4, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 1, 64);
    return v;
}

// One half-wave per ambiguous pair, RU pairs per half-wave and round with their loads issued together: the layout and the
// operation order of pairs_rescore_kernel (scan_pairs.hip), so the cosine has the similar scan's bits.  Instead of a
// record, a qualifying pair is one union.
template <int J>
__global__ void __launch_bounds__(256)
clusters_rescore_kernel(const float* __restrict__ corpus, const uint64_t* __restrict__ amb, uint32_t n, RowIds ids,
                        float min_cos, uint32_t* __restrict__ parent) {
    constexpr int DIM = 128 * J;
    constexpr int RU = J <= 3 ? 4 : 2;
    constexpr int PER = RU * (256 / 32);
    const int tid = threadIdx.x, l32 = tid & 31;
    const uint32_t hw = tid >> 5;
    for (uint32_t i0 = blockIdx.x * PER; i0 < n; i0 += gridDim.x * PER) {  // block-uniform
        uint32_t ra[RU], rb[RU];
        f32x4 q[RU][J], v[RU][J];
#pragma unroll
        for (int u = 0; u < RU; ++u) {
            const uint32_t i = i0 + u * (256 / 32) + hw;  // half-wave uniform
            if (i < n) {
                const uint64_t e = amb[i];
                ra[u] = (uint32_t)e;
                rb[u] = (uint32_t)(e >> 32);
                if (ids.of(ra[u]) > ids.of(rb[u])) {  // the lower id's row is the query (rows ascend with ids: never taken today)
                    const uint32_t s = ra[u]; ra[u] = rb[u]; rb[u] = s;
                }
                const f32x4* qp = reinterpret_cast<const f32x4*>(corpus + (size_t)ra[u] * DIM) + l32;
                const f32x4* xp = reinterpret_cast<const f32x4*>(corpus + (size_t)rb[u] * DIM) + l32;
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
                const float qm = sqrtf(clusters_half_sum(s));
                const float xmag = sqrtf(clusters_half_sum(ss));
                const float d = clusters_half_sum(dot);
                float c = (qm == 0.0f || xmag == 0.0f) ? 0.0f : d / (qm * xmag);
                c = c + 0.0f;  // -0 -> +0, as key_pack leaves every search's cosines
                // strictly above the bound; NaN / Inf cosines are no edge
                if (l32 == 0 && c > min_cos && c < __builtin_huge_valf()) uf_unite(parent, ra[u], rb[u]);
            }
        }
    }
}

template <int J>
int32_t clusters_rescore_impl(const float* d_corpus, const uint64_t* d_amb, uint32_t n, RowIds ids, float min_cos,
                              uint32_t* d_parent, uint32_t blocks, hipStream_t stream) {
    hipLaunchKernelGGL(clusters_rescore_kernel<J>, dim3(blocks), dim3(kPairsRefineThreads), 0, stream, d_corpus, d_amb, n, ids,
                       min_cos, d_parent);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

// label[id - id_base] = the id of the row's root, for every live row (the caller filled label with CS_NO_ID).  A live row
// that is not its own root is a member; the first member to reach a root (mark) counts the class and the root itself.
// totals[0] = classes of two or more, totals[1] = ids in them: sums of integers, the same whatever the order.
__global__ void __launch_bounds__(256)
clusters_label_kernel(uint32_t* __restrict__ parent, uint32_t* __restrict__ mark, uint64_t n_rows,
                      const uint32_t* __restrict__ dead, RowIds ids, uint32_t* __restrict__ label, uint64_t n_labels,
                      unsigned long long* __restrict__ totals) {
    __shared__ uint32_t s_clusters, s_members;
    if (threadIdx.x == 0) { s_clusters = 0u; s_members = 0u; }
    __syncthreads();
    uint32_t clusters = 0, members = 0;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_rows; r += (uint64_t)gridDim.x * 256) {
        if (dead && ((dead[r >> 5] >> (r & 31)) & 1u)) continue;
        const uint32_t root = uf_root(parent, (uint32_t)r);
        // flatten: the root is an ancestor, and other threads' walks through this word stay walks to the same root
        if (root != (uint32_t)r) __hip_atomic_store(parent + r, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t slot = (uint64_t)(ids.of(r) - ids.base);
        if (slot < n_labels) label[slot] = ids.of(root);
        if (root != (uint32_t)r) {
            ++members;
            if (atomicExch(mark + root, 1u) == 0u) { ++clusters; ++members; }
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

uint32_t clusters_row_blocks(uint64_t n_rows) {
    const uint64_t want = (n_rows + 255) / 256;
    return (uint32_t)(want < 1 ? 1 : (want > 65536 ? 65536 : want));
}

}  // namespace

int32_t launch_clusters_init(uint32_t* d_parent, uint32_t* d_mark, uint64_t n_rows, hipStream_t stream) {
    if (n_rows == 0) return CS_OK;
    hipLaunchKernelGGL(clusters_init_kernel, dim3(clusters_row_blocks(n_rows)), dim3(256), 0, stream, d_parent, d_mark, n_rows);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_tile_roots(uint32_t* d_parent, uint64_t tiles, uint64_t n_rows, const uint32_t* d_dead,
                                   uint32_t* d_tile_root, hipStream_t stream) {
    if (tiles == 0) return CS_OK;
    if (tiles * kPairsTileRows < n_rows || tiles > 0x7FFFFFFFull)
        return fail(CS_ERR_BAD_ARG, "similar-clusters tile roots: %llu tiles do not cover %llu rows", (unsigned long long)tiles,
                    (unsigned long long)n_rows);
    hipLaunchKernelGGL(clusters_tile_root_kernel, dim3((uint32_t)tiles), dim3(128), 0, stream, d_parent, n_rows, d_dead,
                       d_tile_root);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_join(const _Float16* d_split, uint32_t dim, uint64_t tiles, uint64_t first, uint64_t count,
                             uint64_t n_rows, const uint32_t* d_dead, RowIds ids, const GroupView& gv, bool other_group,
                             float min_cos, float margin, const float* d_norms, uint32_t* d_parent,
                             const uint32_t* d_tile_root, uint64_t* d_amb, uint64_t* d_counters, uint32_t amb_cap,
                             hipStream_t stream) {
    if (!split_scan_supported(dim)) return fail(CS_ERR_UNSUPPORTED, "similar-clusters join: dim must be 384, 768 or 1024, got %u", dim);
    if (count == 0) return CS_OK;
    if (count > kPairsBandTilePairs || first + count > tile_pairs_of(tiles) || tiles * kPairsTileRows < n_rows ||
        n_rows > 0xFFFFFFFFull || amb_cap < kClustersAmbiguousMin)
        return fail(CS_ERR_BAD_ARG, "similar-clusters join: launch [%llu, +%llu) outside the triangle of %llu tiles",
                    (unsigned long long)first, (unsigned long long)count, (unsigned long long)tiles);
    static PerDeviceOnce attr_set;  // function attributes are per device
    CS_TRY(attr_set.run([&]() -> int32_t {
        CS_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&clusters_join_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   SH_LDS_BYTES));
        return CS_OK;
    }));
    const uint64_t run = PairsPlan::xcd_run(count);
    hipLaunchKernelGGL(clusters_join_kernel, dim3((uint32_t)PairsPlan::band_blocks(count)), dim3(256), SH_LDS_BYTES, stream,
                       d_split, dim / 64, tiles, first, count, run, n_rows, d_dead, ids, gv, other_group ? 1 : 0,
                       min_cos - margin, min_cos + margin, d_norms, d_parent, d_tile_root, d_amb,
                       reinterpret_cast<unsigned long long*>(d_counters), amb_cap);
    CS_HIP(hipGetLastError());
    return CS_OK;
}

int32_t launch_clusters_rescore(const float* d_corpus, uint32_t dim, const uint64_t* d_amb, uint32_t n, RowIds ids, float min_cos,
                                uint32_t* d_parent, uint32_t blocks, hipStream_t stream) {
    if (n == 0) return CS_OK;
    switch (dim) {
        case 384: return clusters_rescore_impl<3>(d_corpus, d_amb, n, ids, min_cos, d_parent, blocks, stream);
        case 768: return clusters_rescore_impl<6>(d_corpus, d_amb, n, ids, min_cos, d_parent, blocks, stream);
        case 1024: return clusters_rescore_impl<8>(d_corpus, d_amb, n, ids, min_cos, d_parent, blocks, stream);
        default: return fail(CS_ERR_UNSUPPORTED, "similar-clusters rescore: dim must be 384, 768 or 1024, got %u", dim);
    }
}

int32_t launch_clusters_label(uint32_t* d_parent, uint32_t* d_mark, uint64_t n_rows, const uint32_t* d_dead, RowIds ids,
                              uint32_t* d_label, uint64_t n_labels, uint64_t* d_totals, hipStream_t stream) {
    if (n_rows == 0) return CS_OK;
    hipLaunchKernelGGL(clusters_label_kernel, dim3(clusters_row_blocks(n_rows)), dim3(256), 0, stream, d_parent, d_mark, n_rows,
                       d_dead, ids, d_label, n_labels, reinterpret_cast<unsigned long long*>(d_totals));
    CS_HIP(hipGetLastError());
    return CS_OK;
}

}  // namespace cs
