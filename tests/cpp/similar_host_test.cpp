// The C++ host mirror's similar-chunk search (codesearch_amd/host/codesearch_gpu.hpp: VectorStore::similar): three files
// in 8-d, one of which holds the source chunk and the three chunks nearest to it.  Built and run by
// tests/test_gpu_similar_search.py with g++ against libcsgpu.so; needs the GPU.
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
    VectorStore store("similar.db", dim);
    // chunk i: e0 + eps_i * e_(1 + i % 7); chunk 0 is e0 itself, so the cosine with it falls as eps grows.  hog.rs holds
    // the source (chunk 0) and the three smallest eps.
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
    auto id_list = [](const std::vector<SearchResult>& rs) {
        std::vector<uint32_t> out;
        for (const auto& r : rs) out.push_back(r.id);
        return out;
    };
    // never the chunk itself; its own file fills the list
    REQUIRE((id_list(store.similar(0, 3)) == std::vector<uint32_t>{2, 4, 6}));
    // no group assigned yet: other_files excludes the chunk alone
    REQUIRE((id_list(store.similar(0, 3, true)) == std::vector<uint32_t>{2, 4, 6}));
    // a chunk's group is its file
    std::map<std::string, uint32_t> number;
    std::vector<uint32_t> groups;
    for (size_t i = 0; i < 9; ++i) groups.push_back(number.emplace(paths[i], (uint32_t)number.size()).first->second);
    store.set_groups(ids, groups);
    REQUIRE((id_list(store.similar(0, 3)) == std::vector<uint32_t>{2, 4, 6}));
    auto other = store.similar(0, 3, true);
    REQUIRE((id_list(other) == std::vector<uint32_t>{1, 3, 5}));
    REQUIRE(other[0].meta.path == "a.rs" && other[1].meta.path == "b.rs" && other[2].meta.path == "a.rs");
    REQUIRE(other[0].score > other[1].score && other[1].score > other[2].score);
    REQUIRE((id_list(store.similar(0, 20, true)) == std::vector<uint32_t>{1, 3, 5, 7, 8}));  // fewer than asked for
    REQUIRE((id_list(store.similar(0, 20)) == std::vector<uint32_t>{2, 4, 6, 1, 3, 5, 7, 8}));
    REQUIRE((id_list(store.similar(3, 2, true)) == std::vector<uint32_t>{0, 2}));  // from b.rs: hog.rs is another file
    // the source is what the plain search of its row finds first
    REQUIRE((id_list(store.search(chunks[0].embedding, 4)) == std::vector<uint32_t>{0, 2, 4, 6}));
    bool threw = false;
    try { store.similar(99, 3); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG; }
    REQUIRE(threw);
    REQUIRE(store.delete_chunks({4}) == 1);
    store.build_index();
    threw = false;
    try { store.similar(4, 3); } catch (const Error& e) { threw = e.code == CS_ERR_BAD_ARG && std::string(e.what()).find("deleted") != std::string::npos; }
    REQUIRE(threw);
    REQUIRE((id_list(store.similar(0, 3)) == std::vector<uint32_t>{2, 6, 1}));
    VectorStore sharded("s.db", dim, std::vector<int32_t>{0, 0}, /*rows_per_stripe=*/4);
    threw = false;
    try { sharded.similar(0, 3); } catch (const Error& e) { threw = e.code == CS_ERR_UNSUPPORTED; }
    REQUIRE(threw);
    std::printf("similar host ok\n");
    return 0;
}
