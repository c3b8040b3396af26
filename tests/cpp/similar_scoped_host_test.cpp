// The C++ host mirror's similar-chunk search inside a scope (codesearch_amd/host/codesearch_gpu.hpp:
// VectorStore::similar(id, limit, other_files, scope)): the three files of similar_host_test.cpp in 8-d and a scope that
// holds part of each.  Built and run by tests/test_gpu_similar_scoped.py with g++ against libcsgpu.so; needs the GPU.
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
    VectorStore store("similar_scoped.db", dim);
    // chunk i: e0 + eps_i * e_(1 + i % 7); chunk 0 is e0 itself.  Two chunks' cosine is 1 / (|a| |b|) unless they share an
    // axis, so from any source the others are ordered by their eps.
    const char* paths[9] = {"hog.rs", "a.rs", "hog.rs", "b.rs", "hog.rs", "a.rs", "hog.rs", "b.rs", "a.rs"};
    const float eps[9] = {0.00f, 0.50f, 0.02f, 0.60f, 0.03f, 0.70f, 0.04f, 0.80f, 0.90f};
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
    std::map<std::string, uint32_t> number;
    std::vector<uint32_t> groups;
    for (size_t i = 0; i < 9; ++i) groups.push_back(number.emplace(paths[i], (uint32_t)number.size()).first->second);
    store.set_groups(ids, groups);
    auto id_list = [](const std::vector<SearchResult>& rs) {
        std::vector<uint32_t> out;
        for (const auto& r : rs) out.push_back(r.id);
        return out;
    };
    {
        VectorStore::Scope sc = store.scope({1, 3, 4, 5, 6, 8});  // hog.rs: 4, 6; a.rs: 1, 5, 8; b.rs: 3
        // the source (chunk 0) is not in the scope; its two nearest chunks (2, then 4) are in its file, 2 outside the scope
        REQUIRE((id_list(store.similar(0, 3, false, sc)) == std::vector<uint32_t>{4, 6, 1}));
        auto other = store.similar(0, 3, true, sc);
        REQUIRE((id_list(other) == std::vector<uint32_t>{1, 3, 5}));
        REQUIRE(other[0].meta.path == "a.rs" && other[1].meta.path == "b.rs" && other[2].meta.path == "a.rs");
        REQUIRE((id_list(store.similar(0, 20, true, sc)) == std::vector<uint32_t>{1, 3, 5, 8}));  // fewer than asked for
        // a source inside the scope is never returned
        REQUIRE((id_list(store.similar(4, 2, false, sc)) == std::vector<uint32_t>{6, 1}));
        REQUIRE((id_list(store.similar(4, 2, true, sc)) == std::vector<uint32_t>{1, 3}));
        uint64_t gathered = 0;
        sc.route_info(nullptr, &gathered, nullptr, nullptr);
        REQUIRE(gathered == 5);
        bool threw = false;
        try { store.similar(99, 3, false, sc); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
        REQUIRE(threw);
        VectorStore sharded("similar_scoped_s.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
        threw = false;
        try { sharded.similar(0, 3, false, sc); } catch (const Error& e) { threw = e.code == CS_ERR_UNSUPPORTED; }
        REQUIRE(threw);
    }
    std::printf("similar scoped host ok\n");
    return 0;
}
