// The C++ host mirror's scoped similar-clusters search (codesearch_amd/host/codesearch_gpu.hpp: the scoped overload of
// VectorStore::similar_clusters): nine chunks in 384-d — chunks 0, 2, 4 are clones of each other through chunk 2 ONLY
// (0 ~ 2 and 2 ~ 4; 0 and 4 are not), chunks 1 and 5 are a clone pair, four chunks alone.  Built and run by
// tests/test_gpu_similar_clusters_scoped.py with g++ against libcsgpu.so; needs the GPU.
#include <cmath>
#include <cstdio>
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
    VectorStore store("clusters_scoped.db", dim);
    std::vector<EmbeddedChunk> chunks(9);
    for (size_t i = 0; i < 9; ++i) {
        chunks[i].chunk.content = "chunk " + std::to_string(i);
        chunks[i].chunk.kind = "Function";
        chunks[i].chunk.path = i < 5 ? "src/a.rs" : "vendor/b.rs";
        chunks[i].embedding.assign(dim, 0.f);
        chunks[i].embedding[200 + i] = 1.f;  // alone unless set below
    }
    // 0 = e0, 4 = e1, 2 = (e0 + e1) / sqrt 2: cos(0, 2) = cos(2, 4) = 0.707, cos(0, 4) = 0
    chunks[0].embedding.assign(dim, 0.f); chunks[0].embedding[0] = 1.f;
    chunks[4].embedding.assign(dim, 0.f); chunks[4].embedding[1] = 1.f;
    chunks[2].embedding.assign(dim, 0.f); chunks[2].embedding[0] = chunks[2].embedding[1] = std::sqrt(0.5f);
    chunks[1].embedding.assign(dim, 0.f); chunks[1].embedding[100] = 1.f; chunks[1].embedding[301] = 0.05f;
    chunks[5].embedding.assign(dim, 0.f); chunks[5].embedding[100] = 1.f; chunks[5].embedding[305] = 0.05f;
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
    const float bound = 0.6f;
    // unscoped: {0, 2, 4} through 2, and {1, 5}
    REQUIRE((id_lists(store.similar_clusters(bound, false, 2, &clusters, &members)) == Lists{{0, 2, 4}, {1, 5}}));
    // a scope of every id, passed as one scope: the same report
    VectorStore::Scope every = store.scope({0, 1, 2, 3, 4, 5, 6, 7, 8});
    REQUIRE((id_lists(store.similar_clusters(every, nullptr, bound, false, 2, &clusters, &members)) == Lists{{0, 2, 4}, {1, 5}}));
    REQUIRE(clusters == 2 && members == 5);
    // NOT a restriction: without chunk 2 the scope holds 0 and 4 alone, and 1 ~ 5 still
    VectorStore::Scope without2 = store.scope({0, 1, 3, 4, 5});
    REQUIRE((id_lists(store.similar_clusters(without2, nullptr, bound, false, 2, &clusters, &members)) == Lists{{1, 5}}));
    REQUIRE(clusters == 1 && members == 2);
    REQUIRE((id_lists(store.similar_clusters(without2, nullptr, bound, false, 1)) == Lists{{1, 5}, {0}, {3}, {4}}));
    // between two scopes: {0, 4} x {2} joins all three; {0, 1} x {4, 5}: only 1 ~ 5 crosses
    VectorStore::Scope ends = store.scope({0, 4}), mid = store.scope({2}), left = store.scope({0, 1}), right = store.scope({4, 5});
    REQUIRE((id_lists(store.similar_clusters(ends, &mid, bound, false, 2, &clusters, &members)) == Lists{{0, 2, 4}}));
    REQUIRE(clusters == 1 && members == 3);
    REQUIRE((id_lists(store.similar_clusters(mid, &ends, bound, false)) == Lists{{0, 2, 4}}));  // swapped: the same
    auto across = store.similar_clusters(left, &right, bound, false, 2, &clusters, &members);
    REQUIRE((id_lists(across) == Lists{{1, 5}}));
    REQUIRE(across[0][0].meta.path == "src/a.rs" && across[0][1].meta.path == "vendor/b.rs" && across[0][1].meta.content == "chunk 5");
    // the same scope named as `other`: the classes inside it
    REQUIRE((id_lists(store.similar_clusters(every, &every, bound, false)) == Lists{{0, 2, 4}, {1, 5}}));
    // an empty join: one id on each side, the same one; and an empty side
    VectorStore::Scope two = store.scope({2}), none = store.scope({});
    REQUIRE(store.similar_clusters(mid, &two, bound, false).empty() && store.similar_clusters(mid, &two, bound, false, 1).size() == 1);
    REQUIRE((id_lists(store.similar_clusters(none, &ends, bound, false, 1)) == Lists{{0}, {4}}));
    VectorStore sharded("s.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
    bool threw = false;
    try { sharded.similar_clusters(every, nullptr, bound); } catch (const Error& e) {
        threw = e.code == CS_ERR_UNSUPPORTED && std::string(e.what()).find("no similar-clusters search") != std::string::npos;
    }
    REQUIRE(threw);
    std::printf("similar clusters scoped host ok\n");
    return 0;
}
