// The host plan of a masked search (codesearch_amd/csrc/masked_plan.hpp) on the CPU: the popcount bound, the mask window,
// the row-list grid and the per-shard restatement of the mask against brute force.
//   masked_plan_test                 -> the checks below, "masked plan ok"
//   masked_plan_test restate S N B X -> reads ceil(B / 32) mask words (u32 little-endian) from stdin and writes, for each
//                                       shard of a store of N shards in stripes of S with next_id X, its local bit count
//                                       (u64) and its words (tests/test_masked_host.py compares them with numpy)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../codesearch_amd/csrc/masked_plan.hpp"

using namespace cs;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            ++failures;                                                   \
        }                                                                 \
    } while (0)

static bool bit(const std::vector<uint32_t>& w, uint64_t i) { return i / 32 < w.size() && ((w[i / 32] >> (i % 32)) & 1u); }

static void check_popcount() {
    std::mt19937_64 rng(7);
    for (int rep = 0; rep < 200; ++rep) {
        const uint64_t bits = 1 + rng() % 2000;
        std::vector<uint32_t> w((bits + 31) / 32);
        for (auto& x : w) x = (uint32_t)rng();
        const uint64_t lo = rng() % (bits + 1), hi = lo + rng() % (bits - lo + 1);
        uint64_t n = 0;
        for (uint64_t i = lo; i < hi; ++i) n += bit(w, i);
        CHECK(popcount_range(w.data(), lo, hi) == n);
    }
    // the bound: only issued ids count, never more than the live rows
    std::vector<uint32_t> all(4, ~0u);  // 128 bits
    CHECK(allowed_bound(all.data(), 128, 0, 100, 100) == 100);
    CHECK(allowed_bound(all.data(), 128, 40, 100, 1000) == 60);   // id_base 40
    CHECK(allowed_bound(all.data(), 50, 40, 100, 1000) == 10);    // a mask shorter than next_id
    CHECK(allowed_bound(all.data(), 128, 0, 100, 30) == 30);      // 30 live rows
    CHECK(allowed_bound(all.data(), 0, 0, 100, 100) == 0);        // allow_bits 0: nothing
    CHECK(allowed_bound(nullptr, 128, 0, 100, 100) == 0);
}

static void check_window() {
    MaskWindow m = mask_window(1000, 0, 600);
    CHECK(m.lo == 0 && m.hi == 600 && m.first_word == 0 && m.words == 19);
    m = mask_window(1000, 70, 600);  // id_base 70: the copy starts at the word holding id 64
    CHECK(m.lo == 64 && m.hi == 600 && m.first_word == 2 && m.words == 17);
    m = mask_window(50, 70, 600);  // the mask ends below the first id
    CHECK(m.words == 0 && m.first_word == 0 && m.lo == 0 && m.hi == 0);
    CHECK(mask_list_blocks(0) == 0 && mask_list_blocks(1) == 1 && mask_list_blocks(4096) == 1 && mask_list_blocks(4097) == 2);
}

static void check_prime() {
    RouteKnobs kn;
    // the streaming route's rule on the bound: no prime pass over a small list, one over millions of rows
    CHECK(masked_prime_rows(kn, 1000, 1, 10, 384, 256, true) == 0);
    CHECK(masked_prime_rows(kn, 10000000, 1, 200, 384, 256, true) > 0);
    CHECK(masked_prime_rows(kn, 10000000, 1, 200, 100, 256, false) == 0);  // no prime kernel for this dim
    kn.prime_min_k = 0;
    CHECK(masked_prime_rows(kn, 10000000, 1, 200, 384, 256, true) == 0);
    // the knobs of tests/test_gpu_scan.py::test_every_scan_kind_returns_the_streaming_scan_bits: its masked and scoped
    // searches over 12,000 allowed rows (11,880 after its deletions) do take the prime pass, over 2,400 list entries
    RouteKnobs forced;
    forced.prime_min_k = 1;
    forced.prime_min_rows = 1;
    forced.prime_rows = 2400;
    for (uint64_t bound : {12000ull, 11880ull})
        for (uint32_t nq : {1u, 2u, 4u})
            for (uint32_t k : {10u, 200u}) {
                for (uint32_t dim : {384u, 768u, 1024u}) CHECK(masked_prime_rows(forced, bound, nq, k, dim, 256, true) == 2400);
                CHECK(masked_prime_rows(forced, bound, nq, k, 100, 256, false) == 0);
            }
}

static void check_shards() {
    std::mt19937_64 rng(11);
    const uint64_t stripes[] = {1, 3, 32, 100, 4096};
    for (uint64_t stripe : stripes)
        for (uint32_t n = 1; n <= 8; ++n)
            for (int rep = 0; rep < 4; ++rep) {
                const uint64_t next = 1 + rng() % 20000;
                const uint64_t bits = rep == 3 ? next + 77 : 1 + rng() % (next + 100);
                std::vector<uint32_t> w((bits + 31) / 32);
                for (auto& x : w) x = (uint32_t)(rng() & rng());
                for (uint32_t s = 0; s < n; ++s) {
                    std::vector<uint32_t> out;
                    uint64_t ob = 0;
                    shard_mask(w.data(), bits, next, stripe, n, s, out, &ob);
                    CHECK(out.size() == (ob + 31) / 32);
                    std::vector<uint8_t> seen(ob, 0);
                    for (uint64_t g = 0; g < next; ++g) {
                        if (shard_of(g, stripe, n) != s) continue;
                        const uint64_t l = shard_local_id(g, stripe, n);
                        const bool want = g < bits && bit(w, g);
                        if (l >= ob) {
                            CHECK(!want);
                            continue;
                        }
                        seen[l] = 1;
                        if (bit(out, l) != want) {
                            std::printf("stripe %llu n %u shard %u id %llu\n", (unsigned long long)stripe, n, s, (unsigned long long)g);
                            CHECK(false);
                            return;
                        }
                    }
                    for (uint64_t l = 0; l < ob; ++l)
                        if (!seen[l]) CHECK(!bit(out, l));  // local ids the store never issued stay clear
                }
            }
}

static int restate(int argc, char** argv) {
    if (argc != 6) return 2;
    const uint64_t stripe = std::strtoull(argv[2], nullptr, 10);
    const uint32_t n = (uint32_t)std::strtoul(argv[3], nullptr, 10);
    const uint64_t bits = std::strtoull(argv[4], nullptr, 10), next = std::strtoull(argv[5], nullptr, 10);
    std::vector<uint32_t> w((bits + 31) / 32);
    if (!w.empty() && std::fread(w.data(), sizeof(uint32_t), w.size(), stdin) != w.size()) return 3;
    for (uint32_t s = 0; s < n; ++s) {
        std::vector<uint32_t> out;
        uint64_t ob = 0;
        shard_mask(w.data(), bits, next, stripe, n, s, out, &ob);
        std::fwrite(&ob, sizeof ob, 1, stdout);
        if (!out.empty()) std::fwrite(out.data(), sizeof(uint32_t), out.size(), stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "restate") == 0) return restate(argc, argv);
    check_popcount();
    check_window();
    check_prime();
    check_shards();
    if (failures) return 1;
    std::printf("masked plan ok\n");
    return 0;
}
