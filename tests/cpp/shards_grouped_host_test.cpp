// The C++ host mirror's grouped search over a sharded store (codesearch_amd/host/codesearch_gpu.hpp: VectorStore::set_groups,
// search_per_file, search_variants_per_file with devices): the three files of tests/cpp/grouped_host_test.cpp dealt over
// three shards in stripes of 2, every call against the same call on one index.  Built and run by
// tests/test_gpu_shards_grouped.py with g++ against libcsgpu.so; needs the GPU.
#include <cstdio>
#include <map>
#include <string>

#include "../../codesearch_amd/host/codesearch_gpu.hpp"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

int main() {
    using namespace cs;
    if (cs_device_count() < 1) { std::printf("no HIP device\n"); return 77; }
    const size_t dim = 8;
    VectorStore single("shards_grouped_single.db", dim);
    VectorStore sharded("shards_grouped_sharded.db", dim, std::vector<int32_t>{0, 0, 0}, /*rows_per_stripe=*/2, /*capacity=*/0,
                        /*grouped=*/true);
    // chunk i: e0 + eps_i * e_(1 + i % 7): cosine with e0 falls as eps grows.  hog.rs holds the four smallest eps.
    const char* paths[9] = {"hog.rs", "a.rs", "hog.rs", "b.rs", "hog.rs", "a.rs", "hog.rs", "b.rs", "a.rs"};
    const float eps[9] = {0.01f, 0.50f, 0.02f, 0.60f, 0.03f, 0.70f, 0.04f, 0.80f, 0.90f};
    std::vector<EmbeddedChunk> chunks(9);
    for (size_t i = 0; i < 9; ++i) {
        chunks[i].chunk.content = "chunk " + std::to_string(i);
        chunks[i].chunk.kind = "Function";
        chunks[i].chunk.path = paths[i];
        chunks[i].embedding.assign(dim, 0.f);
        chunks[i].embedding[0] = 1.f;
        chunks[i].embedding[1 + i % 7] = eps[i];
    }
    const std::vector<uint32_t> ids = single.insert_chunks_with_ids(chunks);
    REQUIRE(sharded.insert_chunks_with_ids(chunks) == ids && ids.size() == 9);
    single.build_index();
    sharded.build_index();
    std::vector<float> q(dim, 0.f), q2(dim, 0.f);
    q[0] = 1.f;
    q2[0] = 1.f;
    q2[2] = 0.3f;
    auto same = [](const std::vector<SearchResult>& a, const std::vector<SearchResult>& b) {
        if (a.size() != b.size()) return false;
        for (size_t i = 0; i < a.size(); ++i)
            if (a[i].id != b[i].id || a[i].score != b[i].score || a[i].meta.path != b[i].meta.path) return false;
        return true;
    };
    auto id_list = [](const std::vector<SearchResult>& rs) {
        std::vector<uint32_t> out;
        for (const auto& r : rs) out.push_back(r.id);
        return out;
    };
    // no group assigned yet: nothing is capped
    REQUIRE(same(sharded.search_per_file(q, 4, 1), single.search_per_file(q, 4, 1)));
    REQUIRE(id_list(sharded.search_per_file(q, 4, 1)) == id_list(sharded.search(q, 4)));
    std::map<std::string, uint32_t> number;
    std::vector<uint32_t> groups;
    for (size_t i = 0; i < 9; ++i) groups.push_back(number.emplace(paths[i], (uint32_t)number.size()).first->second);
    single.set_groups(ids, groups);
    sharded.set_groups(ids, groups);
    REQUIRE((id_list(sharded.search_per_file(q, 4, 1)) == std::vector<uint32_t>{0, 1, 3}));  // each file's best
    REQUIRE((id_list(sharded.search_per_file(q, 5, 2)) == std::vector<uint32_t>{0, 2, 1, 3, 5}));
    for (uint32_t m = 1; m <= 4; ++m) REQUIRE(same(sharded.search_per_file(q, 5, m), single.search_per_file(q, 5, m)));
    REQUIRE(id_list(sharded.search(q, 4)) == (std::vector<uint32_t>{0, 2, 4, 6}));  // the plain search is as it was
    // inside a scope, and over two variants with and without one
    const std::vector<uint32_t> in_scope = {1, 2, 4, 5, 6, 7, 8};
    VectorStore::Scope s1 = single.scope(in_scope), s3 = sharded.scope(in_scope);
    REQUIRE(same(sharded.search_per_file(q, 4, 1, s3), single.search_per_file(q, 4, 1, s1)));
    REQUIRE((id_list(sharded.search_per_file(q, 4, 1, s3)) == std::vector<uint32_t>{2, 1, 7}));
    bool f1 = false, f3 = true;
    REQUIRE(same(sharded.search_variants_per_file({q, q2}, 4, 1, nullptr, &f3), single.search_variants_per_file({q, q2}, 4, 1, nullptr, &f1)));
    REQUIRE(f1 == f3);
    REQUIRE(same(sharded.search_variants_per_file({q, q2}, 4, 2, &s3, &f3), single.search_variants_per_file({q, q2}, 4, 2, &s1, &f1)));
    REQUIRE(f1 == f3);
    bool threw = false;
    try { sharded.search_per_file(q, 4, 0); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    threw = false;
    try { sharded.set_groups({99}, {0}); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    REQUIRE(same(sharded.search_per_file(q, 5, 2), single.search_per_file(q, 5, 2)));  // the refused call assigned nothing
    // a sharded store opened without grouped = true refuses, as it always has
    VectorStore plain("shards_grouped_plain.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
    threw = false;
    try { plain.set_groups({0}, {0}); } catch (const Error& e) { threw = e.code == CS_ERR_UNSUPPORTED; }
    REQUIRE(threw);
    std::printf("shards grouped host ok\n");
    return 0;
}
