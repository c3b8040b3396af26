// The arithmetic of scope algebra (codesearch_amd/csrc/scope_ops_plan.hpp) on the CPU: the diagonal split, the tie rule
// and the per-thread walk are the functions the kernels of scope_ops.hip call; here the tiles are emulated one by one —
// slices copied out with their one neighbour on either side, 256 "threads" of 16 positions each — and the concatenated
// survivors are compared with std::set_union / set_intersection / set_difference.  Stand-alone: g++ -std=c++17, no HIP.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iterator>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/scope_ops_plan.hpp"

using namespace cs;
using Ids = std::vector<uint32_t>;

static int failures = 0;
#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++failures;                                             \
        }                                                           \
    } while (0)

// What the grid computes, block by block; *straddles counts the tiles whose first element is a b that duplicates the a
// before the boundary, or whose last is an a whose twin lies behind it.
static Ids emulate(const Ids& a, const Ids& b, int32_t op, uint64_t* straddles = nullptr) {
    Ids out;
    const uint64_t na = a.size(), nb = b.size(), total = na + nb;
    for (uint64_t t = 0; t < scope_ops_tiles(na, nb); ++t) {
        const uint64_t d0 = t * kScopeOpsTile, d1 = std::min<uint64_t>(d0 + kScopeOpsTile, total);
        const uint64_t i0 = merge_split(a.data(), na, b.data(), nb, d0), i1 = merge_split(a.data(), na, b.data(), nb, d1);
        const uint64_t j0 = d0 - i0, j1 = d1 - i1;
        CHECK(i0 <= i1 && j0 <= j1 && i1 <= na && j1 <= nb);
        const uint32_t nat = (uint32_t)(i1 - i0), nbt = (uint32_t)(j1 - j0), len = (uint32_t)(d1 - d0);
        const bool has_prev = i0 > 0, has_next = j1 < nb;
        // exact-size slices: a read outside what a block loads is an AddressSanitizer report
        Ids sa(a.begin() + (ptrdiff_t)(i0 - has_prev), a.begin() + (ptrdiff_t)i1);
        Ids sb(b.begin() + (ptrdiff_t)j0, b.begin() + (ptrdiff_t)(j1 + has_next));
        const uint32_t* A = sa.data() + has_prev;
        const uint32_t* B = sb.data();
        // the tile's first element is a b (no a of the tile goes before it) that equals the last a of the tile before
        if (straddles && has_prev && nbt && b[j0] == a[i0 - 1] && (nat == 0 || A[0] > b[j0])) ++*straddles;
        for (uint32_t tid = 0; tid < kScopeOpsBlock; ++tid) {
            const uint32_t dt = std::min(tid * kScopeOpsPerThread, len);
            const uint32_t steps = std::min(len - dt, kScopeOpsPerThread);
            const uint32_t ia = (uint32_t)merge_split(A, nat, B, nbt, dt);
            uint32_t vals[kScopeOpsPerThread];
            const uint32_t kept = scope_ops_walk(op, A, nat, has_prev, B, nbt, has_next, ia, dt - ia, steps, vals);
            CHECK(steps == kScopeOpsPerThread || (kept >> steps) == 0);
            for (uint32_t s = 0; s < kScopeOpsPerThread; ++s)
                if ((kept >> s) & 1u) out.push_back(vals[s]);
        }
    }
    return out;
}

static Ids expect(const Ids& a, const Ids& b, int32_t op) {
    Ids out;
    if (op == kScopeOpUnion) std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    else if (op == kScopeOpIntersect) std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    else std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(out));
    return out;
}

static void check_pair(const Ids& a, const Ids& b, uint64_t* straddles = nullptr) {
    for (int32_t op = 0; op < 3; ++op) {
        CHECK(emulate(a, b, op, op == 0 ? straddles : nullptr) == expect(a, b, op));
        CHECK(emulate(b, a, op) == expect(b, a, op));
    }
}

// n distinct ids out of [lo, lo + span), ascending
static Ids random_set(std::mt19937_64& rng, size_t n, uint32_t lo, uint64_t span) {
    Ids v;
    while (v.size() < n) {
        const size_t want = n - v.size();
        for (size_t i = 0; i < want + want / 8 + 4; ++i) v.push_back(lo + (uint32_t)(rng() % span));
        std::sort(v.begin(), v.end());
        v.erase(std::unique(v.begin(), v.end()), v.end());
    }
    // drop random elements down to n (keeps the spread)
    while (v.size() > n) v.erase(v.begin() + (ptrdiff_t)(rng() % v.size()));
    return v;
}

static Ids range(uint32_t first, size_t n, uint32_t step = 1) {
    Ids v(n);
    for (size_t i = 0; i < n; ++i) v[i] = first + (uint32_t)i * step;
    return v;
}

int main() {
    const uint32_t T = kScopeOpsTile;
    static_assert(kScopeOpsTile == kScopeOpsBlock * kScopeOpsPerThread, "a block walks a whole tile");
    static_assert(kScopeOpsPerThread <= 32, "the keep bits of a thread fit one word");
    std::mt19937_64 rng(0x5C09E);

    // the split itself, against a merged sequence with the tie rule spelled out
    {
        const Ids a = random_set(rng, 300, 0, 700), b = random_set(rng, 280, 0, 700);
        std::vector<std::pair<uint32_t, int>> m;
        for (uint32_t x : a) m.push_back({x, 0});
        for (uint32_t y : b) m.push_back({y, 1});
        std::stable_sort(m.begin(), m.end());  // (id, 0 = a) < (id, 1 = b)
        uint64_t from_a = 0;
        for (uint64_t d = 0; d <= m.size(); ++d) {
            CHECK(merge_split(a.data(), a.size(), b.data(), b.size(), d) == from_a);
            if (d < m.size()) from_a += m[d].second == 0;
        }
        CHECK(merge_split(nullptr, 0, b.data(), b.size(), 17) == 0);
        CHECK(merge_split(a.data(), a.size(), nullptr, 0, 17) == 17);
    }

    // lengths 0, 1, tile - 1, tile, tile + 1 (and 3 tile + 1) on both sides: random, equal, interleaved, nested
    const size_t lens[] = {0, 1, T - 1, T, T + 1, 3 * (size_t)T + 1};
    for (size_t la : lens)
        for (size_t lb : lens) {
            check_pair(random_set(rng, la, 0, 4 * (uint64_t)T + 16), random_set(rng, lb, 0, 4 * (uint64_t)T + 16));
            check_pair(range(0, la, 2), range(1, lb, 2));            // disjoint, interleaved
            check_pair(range(5, la), range(5 + (uint32_t)la, lb));   // disjoint, one after the other
            check_pair(range(100, la, 3), range(100, lb, 3));        // one a prefix of the other; equal when la == lb
        }
    {
        const Ids big = random_set(rng, 3 * (size_t)T + 1, 1000, 1u << 20);
        Ids inner;
        for (size_t i = 0; i < big.size(); i += 3) inner.push_back(big[i]);
        check_pair(big, inner);  // one set inside the other
        check_pair(big, big);
    }
    // ids 0 and 0xFFFFFFFF
    {
        Ids a = {0, 7, 0xFFFFFFFFu}, b = {0, 0xFFFFFFFEu, 0xFFFFFFFFu};
        check_pair(a, b);
        check_pair({0}, {0xFFFFFFFFu});
        check_pair({0xFFFFFFFFu}, {0xFFFFFFFFu});
        Ids top = range(0xFFFFFFFFu - (T + 2), T + 3), mid = random_set(rng, T, 0xFFFFFFFFu - 2 * T, 2 * (uint64_t)T + 1);
        CHECK(top.back() == 0xFFFFFFFFu);
        check_pair(top, mid);
    }
    // a duplicate that straddles a tile boundary: equal sets put pair p at positions 2p, 2p + 1, so a shift of one element
    // on the a side puts every a at an odd position and its equal b at the next even one — the last position of a tile and
    // the first of the next, at every boundary
    {
        uint64_t straddles = 0;
        Ids b = range(10, 2 * (size_t)T), a = b;
        a.insert(a.begin(), 3);  // one element of a alone in front
        check_pair(a, b, &straddles);
        CHECK(straddles >= 3);  // (2 T + 1 + 2 T) / T boundaries, each between an a and its equal b
    }
    // random sets over a narrow span (about half of the ids shared), several seeds
    for (int r = 0; r < 6; ++r) {
        uint64_t straddles = 0;
        const size_t la = T + (size_t)(rng() % (2 * T)), lb = T + (size_t)(rng() % (2 * T));
        check_pair(random_set(rng, la, 0, 4 * (uint64_t)T), random_set(rng, lb, 0, 4 * (uint64_t)T), &straddles);
    }

    // striped shards: local ids are dense, a global range is a local range, and local -> global inverts the stripe map
    for (uint32_t nshards : {1u, 3u, 4u})
        for (uint64_t stripe : {1ull, 5ull, 64ull}) {
            std::vector<uint64_t> seen(nshards, 0);
            for (uint64_t g = 0; g < 1000; ++g) {
                const uint32_t s = (uint32_t)((g / stripe) % nshards);
                for (uint32_t o = 0; o < nshards; ++o) CHECK(shard_ids_below(g, stripe, nshards, o) == seen[o]);
                CHECK(shard_global_id(seen[s], stripe, nshards, s) == g);
                ++seen[s];
            }
        }

    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("scope ops plan ok\n");
    return 0;
}
