// The C++ host mirror's grouped search (codesearch_amd/host/codesearch_gpu.hpp: VectorStore::set_groups,
// search_per_file): three files in 8-d, one of which holds the four chunks nearest the query.  Built and run by
// tests/test_gpu_grouped_search.py with g++ against libcsgpu.so; needs the GPU.
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
    VectorStore store("grouped.db", dim);
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
    const std::vector<uint32_t> ids = store.insert_chunks_with_ids(chunks);
    REQUIRE(ids.size() == 9);
    store.build_index();
    std::vector<float> q(dim, 0.f);
    q[0] = 1.f;
    auto id_list = [](const std::vector<SearchResult>& rs) {
        std::vector<uint32_t> out;
        for (const auto& r : rs) out.push_back(r.id);
        return out;
    };
    // no group assigned yet: nothing is capped, and the answer is search()'s
    REQUIRE((id_list(store.search_per_file(q, 4, 1)) == std::vector<uint32_t>{0, 2, 4, 6}));
    REQUIRE(id_list(store.search_per_file(q, 4, 1)) == id_list(store.search(q, 4)));
    // a chunk's group is its file
    std::map<std::string, uint32_t> number;
    std::vector<uint32_t> groups;
    for (size_t i = 0; i < 9; ++i) groups.push_back(number.emplace(paths[i], (uint32_t)number.size()).first->second);
    store.set_groups(ids, groups);
    auto one = store.search_per_file(q, 4, 1);  // three files: three hits, each file's best
    REQUIRE((id_list(one) == std::vector<uint32_t>{0, 1, 3}));
    REQUIRE(one[0].meta.path == "hog.rs" && one[1].meta.path == "a.rs" && one[2].meta.path == "b.rs");
    REQUIRE(one[0].score > one[1].score && one[1].score > one[2].score);
    REQUIRE((id_list(store.search_per_file(q, 5, 2)) == std::vector<uint32_t>{0, 2, 1, 3, 5}));
    REQUIRE(id_list(store.search_per_file(q, 4, 4)) == id_list(store.search(q, 4)));
    REQUIRE(id_list(store.search(q, 4)) == (std::vector<uint32_t>{0, 2, 4, 6}));  // the plain search is as it was
    bool threw = false;
    try { store.search_per_file(q, 4, 0); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    threw = false;
    try { store.set_groups({0, 1}, {0}); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    threw = false;
    try { store.set_groups({99}, {0}); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    VectorStore sharded("s.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
    threw = false;
    try { sharded.search_per_file(q, 4, 1); } catch (const Error& e) { threw = e.code == CS_ERR_UNSUPPORTED; }
    REQUIRE(threw);
    std::printf("grouped host ok\n");
    return 0;
}
