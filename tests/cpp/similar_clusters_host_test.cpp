// The C++ host mirror's similar-clusters search (codesearch_amd/host/codesearch_gpu.hpp: VectorStore::similar_clusters):
// nine chunks in 384-d — a clone class of three over two files, a clone pair inside one file, four chunks alone.  Built and
// run by tests/test_gpu_similar_clusters.py with g++ against libcsgpu.so; needs the GPU.
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
    const size_t dim = 384;
    VectorStore store("clusters.db", dim);
    // chunks 0, 2, 4: e0 + a little of an axis of their own (mutual cosines > 0.99); chunks 1, 5: e100 likewise; the rest
    // one axis each (cosine 0 with everything)
    const char* paths[9] = {"a.rs", "c.rs", "b.rs", "d.rs", "a.rs", "c.rs", "d.rs", "e.rs", "e.rs"};
    const int base[9] = {0, 100, 0, 203, 0, 100, 206, 207, 208};
    std::vector<EmbeddedChunk> chunks(9);
    for (size_t i = 0; i < 9; ++i) {
        chunks[i].chunk.content = "chunk " + std::to_string(i);
        chunks[i].chunk.kind = "Function";
        chunks[i].chunk.path = paths[i];
        chunks[i].embedding.assign(dim, 0.f);
        chunks[i].embedding[base[i]] = 1.f;
        chunks[i].embedding[300 + i] = 0.05f;
    }
    const std::vector<uint32_t> ids = store.insert_chunks_with_ids(chunks);
    REQUIRE(ids.size() == 9);
    store.build_index();
    auto id_lists = [](const std::vector<std::vector<SearchResult>>& cs) {
        std::vector<std::vector<uint32_t>> out;
        for (const auto& c : cs) {
            out.emplace_back();
            for (const auto& r : c) out.back().push_back(r.id);
        }
        return out;
    };
    using Lists = std::vector<std::vector<uint32_t>>;
    uint64_t clusters = 99, members = 99;
    // clones inside files too: the class of three first, then the pair
    REQUIRE((id_lists(store.similar_clusters(0.9f, false, 2, &clusters, &members)) == Lists{{0, 2, 4}, {1, 5}}));
    REQUIRE(clusters == 2 && members == 5);
    // no group assigned yet: other_files drops nothing
    REQUIRE((id_lists(store.similar_clusters(0.9f)) == Lists{{0, 2, 4}, {1, 5}}));
    // a chunk's group is its file: 1 and 5 are one file; 0 and 4 are too, and stay one class through 2
    std::map<std::string, uint32_t> number;
    std::vector<uint32_t> groups;
    for (size_t i = 0; i < 9; ++i) groups.push_back(number.emplace(paths[i], (uint32_t)number.size()).first->second);
    store.set_groups(ids, groups);
    auto across = store.similar_clusters(0.9f, true, 2, &clusters, &members);
    REQUIRE((id_lists(across) == Lists{{0, 2, 4}}));
    REQUIRE(clusters == 1 && members == 3);
    REQUIRE(across[0][0].meta.path == "a.rs" && across[0][1].meta.path == "b.rs" && across[0][1].meta.content == "chunk 2");
    REQUIRE((id_lists(store.similar_clusters(0.9f, false)) == Lists{{0, 2, 4}, {1, 5}}));
    // min_size = 1: the chunks alone come behind, by id; a bound above every cosine leaves nine of them
    REQUIRE((id_lists(store.similar_clusters(0.9f, false, 1)) == Lists{{0, 2, 4}, {1, 5}, {3}, {6}, {7}, {8}}));
    REQUIRE(store.similar_clusters(2.0f, false, 1).size() == 9 && store.similar_clusters(2.0f, false).empty());
    // the smallest member goes: the class is labelled by the next
    REQUIRE(store.delete_chunks({0}) == 1);
    store.build_index();
    REQUIRE((id_lists(store.similar_clusters(0.9f, false, 2, &clusters, &members)) == Lists{{1, 5}, {2, 4}}));
    REQUIRE(clusters == 2 && members == 4);
    VectorStore sharded("s.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
    bool threw = false;
    try { sharded.similar_clusters(0.9f); } catch (const Error& e) {
        threw = e.code == CS_ERR_UNSUPPORTED && std::string(e.what()).find("no similar-clusters search") != std::string::npos;
    }
    REQUIRE(threw);
    std::printf("similar clusters host ok\n");
    return 0;
}
