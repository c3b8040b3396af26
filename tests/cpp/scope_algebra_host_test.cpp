// The C++ host mirror's scope algebra (codesearch_amd/host/codesearch_gpu.hpp: VectorStore::Scope::combine, ::read_ids and
// VectorStore::scope_range) over one index and over a sharded store: forty chunks on the unit axes of a 384-d space, so a
// search for axis i finds chunk i exactly when the scope holds it.  Built and run by tests/test_gpu_scope_algebra.py with g++
// against libcsgpu.so; needs the GPU.
#include <algorithm>
#include <cstdio>
#include <iterator>
#include <string>

#include "../../codesearch_amd/host/codesearch_gpu.hpp"

#define REQUIRE(c)                                                          \
    do {                                                                    \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

using Ids = std::vector<uint32_t>;

static int run(cs::VectorStore& store, const char* what) {
    using namespace cs;
    const size_t dim = 384, n = 40;
    std::vector<EmbeddedChunk> chunks(n);
    for (size_t i = 0; i < n; ++i) {
        chunks[i].chunk.content = "chunk " + std::to_string(i);
        chunks[i].chunk.kind = "Function";
        chunks[i].chunk.path = i < 20 ? "src/a.rs" : "vendor/b.rs";
        chunks[i].embedding.assign(dim, 0.f);
        chunks[i].embedding[i] = 1.f;
    }
    REQUIRE(store.insert_chunks_with_ids(chunks).size() == n);
    store.build_index();
    Ids a, b, every;
    for (uint32_t i = 0; i < n; ++i) {
        every.push_back(i);
        if (i % 3 != 0) a.push_back(i);
        if (i >= 10 && i < 30) b.push_back(i);
    }
    VectorStore::Scope A = store.scope(a), B = store.scope(b);
    REQUIRE(A.read_ids() == a && B.read_ids() == b);
    Ids u, x, d, rest;
    std::set_union(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(u));
    std::set_intersection(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(x));
    std::set_difference(a.begin(), a.end(), b.begin(), b.end(), std::back_inserter(d));
    std::set_difference(every.begin(), every.end(), a.begin(), a.end(), std::back_inserter(rest));
    VectorStore::Scope U = A.combine(B, CS_SCOPE_OP_UNION), X = A.combine(B, CS_SCOPE_OP_INTERSECT),
                       D = A.combine(B, CS_SCOPE_OP_DIFFERENCE);
    REQUIRE(U.read_ids() == u && X.read_ids() == x && D.read_ids() == d);
    VectorStore::Scope all = store.scope_range(0, n);
    REQUIRE(all.read_ids() == every);
    VectorStore::Scope R = all.combine(A, CS_SCOPE_OP_DIFFERENCE);  // everything but A
    REQUIRE(R.read_ids() == rest);
    REQUIRE(store.scope_range(7, 0).read_ids().empty());
    REQUIRE((store.scope_range(38, 5).read_ids() == Ids{38, 39, 40, 41, 42}));  // ids need not be issued
    uint64_t n_ids = 0, live = 0;
    R.info(&n_ids, &live, nullptr);
    REQUIRE(n_ids == rest.size() && live == rest.size());
    // a search for axis i through each scope finds chunk i first exactly when the set holds i
    struct Case { const VectorStore::Scope* sc; const Ids* ids; };
    for (const Case& c : {Case{&U, &u}, Case{&X, &x}, Case{&D, &d}, Case{&R, &rest}}) {
        for (uint32_t i : {0u, 3u, 10u, 11u, 29u, 31u, 39u}) {
            std::vector<float> q(dim, 0.f);
            q[i] = 1.f;
            const auto res = store.search(q, 3, *c.sc);
            const bool held = std::binary_search(c.ids->begin(), c.ids->end(), i);
            REQUIRE(!res.empty() || c.ids->empty());
            REQUIRE((!res.empty() && res[0].id == i) == held);
        }
    }
    // a scope of another store is the library's to refuse
    VectorStore other("scope_algebra_other.db", dim);
    VectorStore::Scope O = other.scope({1, 2});
    bool threw = false;
    try { A.combine(O, CS_SCOPE_OP_UNION); } catch (const Error& e) {
        threw = e.code == CS_ERR_BAD_ARG && std::string(e.what()).find("different stores") != std::string::npos;
    }
    REQUIRE(threw);
    std::printf("%s ok\n", what);
    return 0;
}

int main() {
    using namespace cs;
    if (cs_device_count() < 1) { std::printf("no HIP device\n"); return 77; }
    {
        VectorStore store("scope_algebra.db", 384);
        if (run(store, "one index")) return 1;
    }
    {
        VectorStore sharded("scope_algebra_sharded.db", 384, std::vector<int32_t>{0, 0, 0}, /*rows_per_stripe=*/4);
        if (run(sharded, "sharded")) return 1;
    }
    std::printf("scope algebra host ok\n");
    return 0;
}
