// codesearch_gpu.hpp — header-only C++ mirror of the reference's VectorStore / FastEmbedder
// over the C ABI (include/codesearch_gpu.h), for compiled callers.  Same method names,
// argument meaning and error texts as /root/reference/src/vectordb/store.rs:94-750 and
// src/embed/embedder.rs:201-322; `anyhow::Result<T>` becomes a thrown cs::Error carrying
// the cs_status and the reference-worded message.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <limits>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/codesearch_gpu.h"

namespace cs {

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string& m) : std::runtime_error(m), code(c) {}
};

inline void check(int32_t status) {
    if (status != CS_OK) throw Error(status, cs_last_error());
}

// src/chunker/mod.rs:22-62 (fields that cross into the hot path / its metadata)
struct Chunk {
    std::string content;
    size_t start_line = 0, end_line = 0;
    std::string kind;  // ChunkKind Debug name
    std::string path;
    std::vector<std::string> context;
    std::optional<std::string> signature, docstring;
    std::string hash;
    std::optional<std::string> context_prev, context_next;
};

// src/embed/batch.rs:47-57
struct EmbeddedChunk {
    Chunk chunk;
    std::vector<float> embedding;
};

// store.rs:19-85 (searchable_text omitted: FTS is out of scope)
struct ChunkMetadata {
    std::string content, path;
    size_t start_line = 0, end_line = 0;
    std::string kind;
    std::optional<std::string> signature, docstring, context;
    std::string hash;
    std::optional<std::string> context_prev, context_next;

    static ChunkMetadata from_embedded_chunk(const EmbeddedChunk& ec) {
        ChunkMetadata m;
        const Chunk& c = ec.chunk;
        m.content = c.content; m.path = c.path; m.start_line = c.start_line; m.end_line = c.end_line;
        m.kind = c.kind; m.signature = c.signature; m.docstring = c.docstring; m.hash = c.hash;
        m.context_prev = c.context_prev; m.context_next = c.context_next;
        if (!c.context.empty()) {
            std::string j;
            for (size_t i = 0; i < c.context.size(); ++i) j += (i ? " > " : "") + c.context[i];
            m.context = j;
        }
        return m;
    }
};

// store.rs:753-772
struct SearchResult {
    uint32_t id = 0;
    ChunkMetadata meta;
    float distance = 0.f;  // arroy Cosine: (1 - cos) / 2
    float score = 0.f;     // 1 - distance (store.rs:478)
};

// store.rs:784-792
struct StoreStats {
    size_t total_chunks = 0, total_files = 0;
    bool indexed = false;
    size_t dimensions = 0;
    uint32_t max_chunk_id = 0;
};

class VectorStore {
  public:
    // VectorStore::new(db_path, dimensions) — store.rs:110-176 (db_path unused: nothing persists)
    VectorStore(const std::string& /*db_path*/, size_t dimensions, int device = 0, uint64_t capacity = 0,
                uint32_t id_base = 0)
        : dimensions_(dimensions), id_base_(id_base) {
        check(cs_index_create((uint32_t)dimensions, capacity, device, id_base, &h_));
    }
    // The same store row-sharded over several GPUs of the node inside this process (cs_shards_*):
    // ids stay contiguous, rows are dealt in stripes of rows_per_stripe ids, a search scans every shard and merges
    // on devices[0].  grouped = true: the store keeps groups (set_groups, search_per_file, search_variants_per_file go to
    // cs_shards_set_groups and cs_shards_search_grouped & co.: 8 B per id); without it a sharded store refuses them.
    VectorStore(const std::string& /*db_path*/, size_t dimensions, const std::vector<int32_t>& devices,
                uint64_t rows_per_stripe = 65536, uint64_t capacity = 0, bool grouped = false)
        : dimensions_(dimensions), grouped_(grouped) {
        check(cs_shards_create((uint32_t)dimensions, (uint32_t)devices.size(), devices.data(), rows_per_stripe, capacity, &sh_));
    }
    ~VectorStore() { if (sh_) cs_shards_destroy(sh_); else cs_index_destroy(h_); }
    VectorStore(const VectorStore&) = delete;
    VectorStore& operator=(const VectorStore&) = delete;
    bool sharded() const { return sh_ != nullptr; }
    cs_shards* shards_handle() const { return sh_; }
    // metadata of chunks whose vectors were appended by EmbedderReplicas::index_texts (ids assigned there)
    void put_metadata(const std::vector<uint32_t>& ids, const std::vector<Chunk>& chunks) {
        for (size_t i = 0; i < ids.size() && i < chunks.size(); ++i) {
            EmbeddedChunk ec;
            ec.chunk = chunks[i];
            meta_[ids[i]] = ChunkMetadata::from_embedded_chunk(ec);
        }
    }

    // store.rs:618-686
    std::vector<uint32_t> insert_chunks_with_ids(const std::vector<EmbeddedChunk>& chunks) {
        if (chunks.empty()) return {};
        std::vector<float> rows;
        rows.reserve(chunks.size() * dimensions_);
        for (const auto& c : chunks) {
            if (c.embedding.size() != dimensions_)  // store.rs:666-672
                throw Error(CS_ERR_DIM_MISMATCH, "Embedding dimension mismatch: expected " +
                                                     std::to_string(dimensions_) + ", got " +
                                                     std::to_string(c.embedding.size()));
            rows.insert(rows.end(), c.embedding.begin(), c.embedding.end());
        }
        std::vector<uint32_t> ids(chunks.size());
        check(sh_ ? cs_shards_add(sh_, rows.data(), chunks.size(), (uint32_t)dimensions_, ids.data())
                  : cs_index_add(h_, rows.data(), chunks.size(), (uint32_t)dimensions_, ids.data()));
        for (size_t i = 0; i < chunks.size(); ++i) meta_[ids[i]] = ChunkMetadata::from_embedded_chunk(chunks[i]);
        return ids;
    }
    // store.rs:334-379
    size_t insert_chunks(const std::vector<EmbeddedChunk>& chunks) { return insert_chunks_with_ids(chunks).size(); }
    // store.rs:386-430
    void build_index() { check(sh_ ? cs_shards_build(sh_) : cs_index_build(h_)); }
    // store.rs:548-610
    size_t delete_chunks(const std::vector<uint32_t>& ids) {
        uint64_t removed = 0;
        check(sh_ ? cs_shards_remove(sh_, ids.data(), ids.size(), &removed) : cs_index_remove(h_, ids.data(), ids.size(), &removed));
        for (uint32_t id : ids) meta_.erase(id);
        return (size_t)removed;
    }
    // store.rs:690-707
    void clear() { check(sh_ ? cs_shards_clear(sh_) : cs_index_clear(h_)); meta_.clear(); }
    // store.rs:745
    bool is_indexed() const { return (sh_ ? cs_shards_is_built(sh_) : cs_index_is_built(h_)) != 0; }

    // the mask of a masked search: bit id of word id / 32 for every allowed id below next_id; *bits = next_id
    std::vector<uint32_t> allow_mask(const std::vector<uint32_t>& allowed_ids, uint64_t* bits) const {
        const uint64_t next = sh_ ? cs_shards_next_id(sh_) : cs_index_next_id(h_);
        std::vector<uint32_t> mask((size_t)((next + 31) / 32), 0u);
        for (uint32_t id : allowed_ids)
            if (id < next) mask[id >> 5] |= 1u << (id & 31);
        *bits = mask.empty() ? 0 : next;
        return mask;
    }
    // score != null: the results' scores when they are not 1 - distance (a boosted search's)
    std::vector<SearchResult> results(const std::vector<float>& cos, const std::vector<uint32_t>& ids, uint32_t count,
                                      const std::vector<float>* score = nullptr) const {
        std::vector<SearchResult> out;
        for (uint32_t j = 0; j < count; ++j) {
            auto it = meta_.find(ids[j]);
            if (it == meta_.end()) continue;  // store.rs:465
            SearchResult r;
            r.id = ids[j];
            r.meta = it->second;
            r.distance = cs_cos_to_distance(cos[j]);
            r.score = score ? (*score)[j] : 1.0f - r.distance;
            out.push_back(std::move(r));
        }
        return out;
    }

    // store.rs:431-486
    std::vector<SearchResult> search(const std::vector<float>& query_embedding, size_t limit) const {
        auto all = search_batch({query_embedding}, limit);
        return all.empty() ? std::vector<SearchResult>{} : all[0];
    }
    // filter_path done exactly (src/mcp/mod.rs:251-252,400-425): the best `limit` among the chunks `allowed_ids` names
    // (cs_index_search_masked / cs_shards_search_masked)
    std::vector<SearchResult> search(const std::vector<float>& query_embedding, size_t limit,
                                     const std::vector<uint32_t>& allowed_ids) const {
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        uint64_t bits = 0;
        const std::vector<uint32_t> mask = allow_mask(allowed_ids, &bits);
        const uint32_t dim = (uint32_t)query_embedding.size();
        check(sh_ ? cs_shards_search_masked(sh_, query_embedding.data(), 1, dim, (uint32_t)limit, mask.data(), bits,
                                            cos.data(), ids.data(), counts.data())
                  : cs_index_search_masked(h_, query_embedding.data(), 1, dim, (uint32_t)limit, mask.data(), bits,
                                           cos.data(), ids.data(), counts.data()));
        return results(cos, ids, counts[0]);
    }
    // `--per-file` done exactly (src/search/mod.rs:1007-1038 caps after ranking): the best `limit` chunks with at most
    // `per_file` of one group, decided on the device (cs_index_search_grouped).  A chunk's group is its file once
    // set_groups has said so; chunks without a group are never capped.  One index only: no sharded form yet.
    void set_groups(const std::vector<uint32_t>& ids, const std::vector<uint32_t>& groups) {
        needs_groups();
        if (ids.size() != groups.size()) throw Error(CS_ERR_BAD_ARG, "ids and groups of unequal length");
        check(sh_ ? cs_shards_set_groups(sh_, ids.data(), groups.data(), ids.size())
                  : cs_index_set_groups(h_, ids.data(), groups.data(), ids.size()));
    }
    std::vector<SearchResult> search_per_file(const std::vector<float>& query_embedding, size_t limit,
                                              uint32_t per_file) const {
        needs_groups();
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        const uint32_t dim = (uint32_t)query_embedding.size();
        check(sh_ ? cs_shards_search_grouped(sh_, query_embedding.data(), 1, dim, (uint32_t)limit, per_file, cos.data(), ids.data(),
                                             counts.data())
                  : cs_index_search_grouped(h_, query_embedding.data(), 1, dim, (uint32_t)limit, per_file, cos.data(), ids.data(),
                                            counts.data()));
        return results(cos, ids, counts[0]);
    }
    // The kind and language boosts done exactly (src/search/mod.rs:238-252, :789-806 multiply the scores of hits already
    // ranked): every chunk id may carry a 16-bit class (set_classes; CS_NO_CLASS un-assigns), a call brings one weight per
    // class, and the best `limit` chunks by f32(score * weight), then id, are selected on the device
    // (cs_index_search_boosted; with a Scope, cs_index_search_boosted_scoped).  A chunk without a class, or with a class
    // past the table, weighs 1.  SearchResult::score is the boosted score, ::distance the chunk's own.  One index only.
    void set_classes(const std::vector<uint32_t>& ids, const std::vector<uint16_t>& classes) {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no boosted search");
        if (ids.size() != classes.size()) throw Error(CS_ERR_BAD_ARG, "ids and classes of unequal length");
        check(cs_index_set_classes(h_, ids.data(), classes.data(), ids.size()));
    }
    // (search_boosted itself follows Scope, below)
    // "More like this": the `limit` stored chunks nearest to chunk `id`'s stored row, never the chunk itself; other_files:
    // none of its group (its file, set_groups) either.  The row is gathered and the exclusion applied on the device
    // (cs_index_search_similar), not on a ranked list.  One index only: no sharded form yet.
    std::vector<SearchResult> similar(uint32_t id, size_t limit, bool other_files = false) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search");
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        check(cs_index_search_similar(h_, &id, 1, (uint32_t)limit, other_files ? CS_SIMILAR_EXCLUDE_GROUP : CS_SIMILAR_EXCLUDE_SELF,
                                      -std::numeric_limits<float>::infinity(), cos.data(), ids.data(), counts.data()));
        return results(cos, ids, counts[0]);
    }
    // CS_SIMILAR_ROUTE_AUTO / _SCAN / _FILTER for similar() without a scope (cs_index_set_similar_route): same bits on every
    // route.  similar_route_info: calls the filter answered, calls the scan answered, filter calls the scan had to finish.
    void set_similar_route(int32_t route) {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search");
        check(cs_index_set_similar_route(h_, route));
    }
    struct SimilarRouteInfo {
        uint64_t filter_searches, scan_searches, filter_fallbacks;
    };
    SimilarRouteInfo similar_route_info() const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search");
        SimilarRouteInfo i{0, 0, 0};
        check(cs_index_similar_route_info(h_, &i.filter_searches, &i.scan_searches, &i.filter_fallbacks));
        return i;
    }
    // The near-duplicate report: every pair of stored chunks a < b whose cosine is strictly above min_cos, best first by
    // (cosine desc, a asc, b asc); other_files: never two chunks of one group (file).  The corpus is joined with itself on
    // the device, exactly (cs_index_similar_pairs).  At most max_pairs pairs come back; *total (optional) = how many there
    // are.  Throws CS_ERR_UNSUPPORTED when the bound is so low that more than 2 * max_pairs + 4096 pairs come near it.
    struct SimilarPair {
        uint32_t a, b;
        float cosine;
    };
    std::vector<SimilarPair> similar_pairs(float min_cos, bool other_files = true, uint32_t max_pairs = 65536,
                                           uint64_t* total = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-pairs search");
        std::vector<uint32_t> a(max_pairs), b(max_pairs);
        std::vector<float> cos(max_pairs);
        uint64_t n = 0;
        check(cs_index_similar_pairs(h_, min_cos, other_files ? CS_PAIRS_OTHER_GROUP : CS_PAIRS_ALL, max_pairs, a.data(),
                                     b.data(), cos.data(), &n));
        if (total) *total = n;
        std::vector<SimilarPair> out((size_t)(n < max_pairs ? n : max_pairs));
        for (size_t i = 0; i < out.size(); ++i) out[i] = SimilarPair{a[i], b[i], cos[i]};
        return out;
    }
    // The duplicate-code report by clone class (cs_index_similar_clusters): the connected components of the graph whose
    // edges are the pairs similar_pairs(min_cos, other_files) would return — however many those are: there is no max_pairs
    // and no refusal.  Classes of at least min_size chunks, the largest first, then by label (the smallest id of the
    // class); members by id.  A member's distance and score are a chunk's against itself: a class carries no cosine.
    // Chunks without metadata are skipped; a class is sized by what remains.  *clusters / *members (optional): the classes
    // of two or more ids and the ids in them, as the device counted them.
    std::vector<std::vector<SearchResult>> similar_clusters(float min_cos, bool other_files = true, size_t min_size = 2,
                                                            uint64_t* clusters = nullptr, uint64_t* members = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-clusters search: no cs_shards_ form yet");
        std::vector<uint32_t> label((size_t)(cs_index_next_id(h_) - id_base_), (uint32_t)CS_NO_ID);
        check(cs_index_similar_clusters(h_, min_cos, other_files ? CS_PAIRS_OTHER_GROUP : CS_PAIRS_ALL, label.data(),
                                        label.size(), clusters, members));
        std::map<uint32_t, std::vector<uint32_t>> by_label;  // ascending labels, members ascending
        for (size_t i = 0; i < label.size(); ++i)
            if (label[i] != CS_NO_ID) by_label[label[i]].push_back(id_base_ + (uint32_t)i);
        std::vector<std::vector<SearchResult>> out;
        for (const auto& kv : by_label) {
            std::vector<SearchResult> rs = results(std::vector<float>(kv.second.size(), 1.0f), kv.second, (uint32_t)kv.second.size());
            if (rs.size() >= (min_size ? min_size : 1)) out.push_back(std::move(rs));
        }
        std::stable_sort(out.begin(), out.end(), [](const std::vector<SearchResult>& x, const std::vector<SearchResult>& y) {
            return x.size() > y.size();
        });
        return out;
    }
    // all query variants in one call (src/search/mod.rs:508-511)
    std::vector<std::vector<SearchResult>> search_batch(const std::vector<std::vector<float>>& queries,
                                                        size_t limit) const {
        const size_t nq = queries.size();
        if (nq == 0) return {};
        const size_t qdim = queries[0].size();
        std::vector<float> q;
        for (const auto& v : queries) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> cos(nq * limit);
        std::vector<uint32_t> ids(nq * limit), counts(nq);
        check(sh_ ? cs_shards_search(sh_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, cos.data(), ids.data(),
                                     counts.data())
                  : cs_index_search(h_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, cos.data(), ids.data(),
                                    counts.data()));
        std::vector<std::vector<SearchResult>> out(nq);
        for (size_t i = 0; i < nq; ++i)
            for (uint32_t j = 0; j < counts[i]; ++j) {
                auto it = meta_.find(ids[i * limit + j]);
                if (it == meta_.end()) continue;  // store.rs:465
                SearchResult r;
                r.id = ids[i * limit + j];
                r.meta = it->second;
                r.distance = cs_cos_to_distance(cos[i * limit + j]);
                r.score = 1.0f - r.distance;
                out[i].push_back(std::move(r));
            }
        return out;
    }
    // search::search's vector leg in one call (src/search/mod.rs:508-611): every variant searched for `limit` rows, a
    // chunk found by several variants keeps its best score, the best `limit` distinct chunks best-first — merged on the
    // device; *high_confidence = the top five all have distance < 0.15 (the reference then skips its FTS leg).
    // search_variants over the chunks `allowed_ids` names (cs_index_search_variants_masked)
    std::vector<SearchResult> search_variants(const std::vector<std::vector<float>>& variants, size_t limit,
                                              const std::vector<uint32_t>& allowed_ids,
                                              bool* high_confidence = nullptr) const {
        const size_t nq = variants.size();
        if (nq == 0) return {};
        const size_t qdim = variants[0].size();
        std::vector<float> q;
        for (const auto& v : variants) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit);
        uint32_t count = 0;
        int32_t flag = 0;
        uint64_t bits = 0;
        const std::vector<uint32_t> mask = allow_mask(allowed_ids, &bits);
        check(sh_ ? cs_shards_search_variants_masked(sh_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit,
                                                     mask.data(), bits, cos.data(), ids.data(), &count, &flag)
                  : cs_index_search_variants_masked(h_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, mask.data(),
                                                    bits, cos.data(), ids.data(), &count, &flag));
        if (high_confidence) *high_confidence = flag != 0;
        return results(cos, ids, count);
    }
    // A prepared set of chunk ids of this store (cs_scope): the ids and the row list made from them live on the device,
    // and a search through it returns what the masked search over the same ids returns, with no mask to build, copy or
    // compact per call.  The row list follows the store by itself (the first search after a build remakes it); the id
    // list is fixed.  RAII; a Scope must go before its store.
    class Scope {
      public:
        Scope(const VectorStore& st, std::vector<uint32_t> ids) {
            std::sort(ids.begin(), ids.end());  // the ABI wants strictly ascending ids
            ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
            check(st.sh_ ? cs_shards_scope_create(st.sh_, ids.data(), ids.size(), &h_)
                         : cs_index_scope_create(st.h_, ids.data(), ids.size(), &h_));
        }
        ~Scope() { cs_scope_destroy(h_); }
        Scope(Scope&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
        Scope& operator=(Scope&& o) noexcept {
            if (this != &o) { cs_scope_destroy(h_); h_ = o.h_; o.h_ = nullptr; }
            return *this;
        }
        Scope(const Scope&) = delete;
        Scope& operator=(const Scope&) = delete;
        cs_scope* handle() const { return h_; }
        // ids held, rows of the list as last made, makings of the list (cs_scope_info)
        void info(uint64_t* n_ids, uint64_t* live_rows, uint64_t* refreshes) const {
            check(cs_scope_info(h_, n_ids, live_rows, refreshes));
        }
        // CS_SCOPE_ROUTE_AUTO / _GATHER / _FILTER for this scope's host-buffer searches (cs_scope_set_route)
        void set_route(int32_t route) { check(cs_scope_set_route(h_, route)); }
        // searches through the filter / by the gathered scan, overflow reruns, HBM bytes beyond 8 per id (cs_scope_route_info)
        void route_info(uint64_t* filter_searches, uint64_t* gathered_searches, uint64_t* overflow_reruns,
                        uint64_t* extra_bytes) const {
            check(cs_scope_route_info(h_, filter_searches, gathered_searches, overflow_reruns, extra_bytes));
        }
        // Scope algebra on the device (cs_scope_combine): a new Scope of the same store holding the union (CS_SCOPE_OP_UNION),
        // the intersection (_INTERSECT) or the difference (_DIFFERENCE: this minus other) of the two id sets.  It answers as
        // a Scope made from the host-computed set would; the operands are only read.
        Scope combine(const Scope& other, int32_t op) const {
            Scope out;
            check(cs_scope_combine(h_, other.h_, op, &out.h_));
            return out;
        }
        // the scope's id set, ascending (global ids over a sharded store): cs_scope_read_ids
        std::vector<uint32_t> read_ids() const {
            uint64_t n = 0;
            check(cs_scope_info(h_, &n, nullptr, nullptr));
            std::vector<uint32_t> ids((size_t)n);
            check(cs_scope_read_ids(h_, 0, n, ids.data()));
            return ids;
        }

      private:
        friend class VectorStore;
        Scope() = default;
        cs_scope* h_ = nullptr;
    };
    Scope scope(std::vector<uint32_t> ids) const { return Scope(*this, std::move(ids)); }
    // The scope of ids [first_id, first_id + n), written on the device (cs_index_scope_create_range / cs_shards_): with
    // combine(), "everything but x" is scope_range(id_base, next_id - id_base).combine(x, CS_SCOPE_OP_DIFFERENCE).
    Scope scope_range(uint32_t first_id, uint64_t n) const {
        Scope out;
        check(sh_ ? cs_shards_scope_create_range(sh_, first_id, n, &out.h_) : cs_index_scope_create_range(h_, first_id, n, &out.h_));
        return out;
    }
    // search / search_variants over a prepared Scope (cs_index_search_scoped / cs_index_search_variants_scoped & the
    // cs_shards_ forms)
    std::vector<SearchResult> search(const std::vector<float>& query_embedding, size_t limit, const Scope& scope) const {
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        const uint32_t dim = (uint32_t)query_embedding.size();
        check(sh_ ? cs_shards_search_scoped(sh_, scope.handle(), query_embedding.data(), 1, dim, (uint32_t)limit, cos.data(),
                                            ids.data(), counts.data())
                  : cs_index_search_scoped(h_, scope.handle(), query_embedding.data(), 1, dim, (uint32_t)limit, cos.data(),
                                           ids.data(), counts.data()));
        return results(cos, ids, counts[0]);
    }
    std::vector<SearchResult> search_variants(const std::vector<std::vector<float>>& variants, size_t limit,
                                              const Scope& scope, bool* high_confidence = nullptr) const {
        const size_t nq = variants.size();
        if (nq == 0) return {};
        const size_t qdim = variants[0].size();
        std::vector<float> q;
        for (const auto& v : variants) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit);
        uint32_t count = 0;
        int32_t flag = 0;
        check(sh_ ? cs_shards_search_variants_scoped(sh_, scope.handle(), q.data(), (uint32_t)nq, (uint32_t)qdim,
                                                     (uint32_t)limit, cos.data(), ids.data(), &count, &flag)
                  : cs_index_search_variants_scoped(h_, scope.handle(), q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit,
                                                    cos.data(), ids.data(), &count, &flag));
        if (high_confidence) *high_confidence = flag != 0;
        return results(cos, ids, count);
    }
    // `--per-file` inside a Scope, and over the merged query variants with or without one (cs_index_search_grouped_scoped,
    // cs_index_search_variants_grouped, cs_index_search_variants_grouped_scoped): the cap is applied on the device, to the
    // scope's rows and to the merged order; the flag is the predicate on the capped list.  One index only.
    std::vector<SearchResult> search_per_file(const std::vector<float>& query_embedding, size_t limit, uint32_t per_file,
                                              const Scope& scope) const {
        needs_groups();
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        const uint32_t dim = (uint32_t)query_embedding.size();
        check(sh_ ? cs_shards_search_grouped_scoped(sh_, scope.handle(), query_embedding.data(), 1, dim, (uint32_t)limit, per_file,
                                                    cos.data(), ids.data(), counts.data())
                  : cs_index_search_grouped_scoped(h_, scope.handle(), query_embedding.data(), 1, dim, (uint32_t)limit, per_file,
                                                   cos.data(), ids.data(), counts.data()));
        return results(cos, ids, counts[0]);
    }
    // The boosted search (set_classes, above) over the whole store or, with `scope`, over its chunks.
    std::vector<SearchResult> search_boosted(const std::vector<float>& query_embedding, size_t limit,
                                             const std::vector<float>& class_weights, const Scope* scope = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no boosted search");
        std::vector<float> score(limit), cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        const uint32_t dim = (uint32_t)query_embedding.size(), nc = (uint32_t)class_weights.size();
        check(scope ? cs_index_search_boosted_scoped(h_, scope->handle(), query_embedding.data(), 1, dim, (uint32_t)limit,
                                                     class_weights.data(), nc, score.data(), cos.data(), ids.data(), counts.data())
                    : cs_index_search_boosted(h_, query_embedding.data(), 1, dim, (uint32_t)limit, class_weights.data(), nc,
                                              score.data(), cos.data(), ids.data(), counts.data()));
        std::vector<SearchResult> out = results(cos, ids, counts[0], &score);
        return out;
    }
    // The boosted search over the merged query variants — a chunk keeps its best cosine, and so its best boosted score —
    // with or without a Scope, and with per_file != 0 under the per-file cap, all decided on the device
    // (cs_index_search_variants_boosted and its _scoped / _grouped / _grouped_scoped forms): what one reference search
    // computes.  The flag is the predicate on the returned list's cosines.  One index only.
    std::vector<SearchResult> search_variants_boosted(const std::vector<std::vector<float>>& variants, size_t limit,
                                                      const std::vector<float>& class_weights, uint32_t per_file = 0,
                                                      const Scope* scope = nullptr, bool* high_confidence = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no boosted search");
        const size_t nq = variants.size();
        if (nq == 0) return {};
        const size_t qdim = variants[0].size();
        std::vector<float> q;
        for (const auto& v : variants) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> score(limit), cos(limit);
        std::vector<uint32_t> ids(limit);
        uint32_t count = 0;
        int32_t flag = 0;
        const uint32_t n = (uint32_t)nq, dim = (uint32_t)qdim, k = (uint32_t)limit, nc = (uint32_t)class_weights.size();
        const float* w = class_weights.data();
        if (per_file)
            check(scope ? cs_index_search_variants_boosted_grouped_scoped(h_, scope->handle(), q.data(), n, dim, k, per_file, w, nc,
                                                                          score.data(), cos.data(), ids.data(), &count, &flag)
                        : cs_index_search_variants_boosted_grouped(h_, q.data(), n, dim, k, per_file, w, nc, score.data(),
                                                                   cos.data(), ids.data(), &count, &flag));
        else
            check(scope ? cs_index_search_variants_boosted_scoped(h_, scope->handle(), q.data(), n, dim, k, w, nc, score.data(),
                                                                  cos.data(), ids.data(), &count, &flag)
                        : cs_index_search_variants_boosted(h_, q.data(), n, dim, k, w, nc, score.data(), cos.data(), ids.data(),
                                                           &count, &flag));
        if (high_confidence) *high_confidence = flag != 0;
        return results(cos, ids, count, &score);
    }
    // similar() among the chunks of a Scope only (cs_index_search_similar_scoped): "where else under src/ is this copied".
    // Chunk `id` itself need not be in the scope.  One index only.  The scope's route (cs_scope_set_route) picks the gathered
    // scan or the int8 filter planned over the scope's rows; the results are the same.
    std::vector<SearchResult> similar(uint32_t id, size_t limit, bool other_files, const Scope& scope) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-chunk search");
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit), counts(1);
        check(cs_index_search_similar_scoped(h_, scope.handle(), &id, 1, (uint32_t)limit,
                                             other_files ? CS_SIMILAR_EXCLUDE_GROUP : CS_SIMILAR_EXCLUDE_SELF,
                                             -std::numeric_limits<float>::infinity(), cos.data(), ids.data(), counts.data()));
        return results(cos, ids, counts[0]);
    }
    // similar_pairs() inside `scope` (other == nullptr) or between `scope` and `*other`: every pair with one chunk in each
    // scope, once however the two overlap, with the bytes the unscoped call gives (cs_index_similar_pairs_scoped).  The
    // candidate bound counts those pairs only.  One index only.
    std::vector<SimilarPair> similar_pairs(const Scope& scope, const Scope* other, float min_cos, bool other_files = true,
                                           uint32_t max_pairs = 65536, uint64_t* total = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-pairs search");
        std::vector<uint32_t> a(max_pairs), b(max_pairs);
        std::vector<float> cos(max_pairs);
        uint64_t n = 0;
        check(cs_index_similar_pairs_scoped(h_, scope.handle(), other ? other->handle() : scope.handle(), min_cos,
                                            other_files ? CS_PAIRS_OTHER_GROUP : CS_PAIRS_ALL, max_pairs, a.data(), b.data(),
                                            cos.data(), &n));
        if (total) *total = n;
        std::vector<SimilarPair> out((size_t)(n < max_pairs ? n : max_pairs));
        for (size_t i = 0; i < out.size(); ++i) out[i] = SimilarPair{a[i], b[i], cos[i]};
        return out;
    }
    // similar_clusters() inside `scope` (other == nullptr) or of the pairs between `scope` and `*other`
    // (cs_index_similar_clusters_scoped): the vertices are the live ids of the two scopes and an edge needs one end in
    // each.  NOT the unscoped classes restricted to the scope: a path through a chunk outside connects nothing.  Never
    // refused for abundance.  The report's shape is the unscoped overload's.  One index only.
    std::vector<std::vector<SearchResult>> similar_clusters(const Scope& scope, const Scope* other, float min_cos,
                                                            bool other_files = true, size_t min_size = 2,
                                                            uint64_t* clusters = nullptr, uint64_t* members = nullptr) const {
        if (sh_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no similar-clusters search: no cs_shards_ form yet");
        const bool same = !other || other->handle() == scope.handle();
        uint64_t cap = 0, nb = 0;
        check(cs_scope_info(scope.handle(), &cap, nullptr, nullptr));
        if (!same) check(cs_scope_info(other->handle(), &nb, nullptr, nullptr));
        cap += nb;
        std::vector<uint32_t> ids((size_t)cap), label((size_t)cap);
        uint64_t n = 0;
        check(cs_index_similar_clusters_scoped(h_, scope.handle(), same ? scope.handle() : other->handle(), min_cos,
                                               other_files ? CS_PAIRS_OTHER_GROUP : CS_PAIRS_ALL, ids.data(), label.data(), cap,
                                               &n, clusters, members));
        std::map<uint32_t, std::vector<uint32_t>> by_label;  // ascending labels, members ascending
        for (size_t i = 0; i < (size_t)n; ++i) by_label[label[i]].push_back(ids[i]);
        std::vector<std::vector<SearchResult>> out;
        for (const auto& kv : by_label) {
            std::vector<SearchResult> rs = results(std::vector<float>(kv.second.size(), 1.0f), kv.second, (uint32_t)kv.second.size());
            if (rs.size() >= (min_size ? min_size : 1)) out.push_back(std::move(rs));
        }
        std::stable_sort(out.begin(), out.end(), [](const std::vector<SearchResult>& x, const std::vector<SearchResult>& y) {
            return x.size() > y.size();
        });
        return out;
    }
    std::vector<SearchResult> search_variants_per_file(const std::vector<std::vector<float>>& variants, size_t limit,
                                                       uint32_t per_file, const Scope* scope = nullptr,
                                                       bool* high_confidence = nullptr) const {
        needs_groups();
        const size_t nq = variants.size();
        if (nq == 0) return {};
        const size_t qdim = variants[0].size();
        std::vector<float> q;
        for (const auto& v : variants) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit);
        uint32_t count = 0;
        int32_t flag = 0;
        if (sh_)
            check(scope ? cs_shards_search_variants_grouped_scoped(sh_, scope->handle(), q.data(), (uint32_t)nq, (uint32_t)qdim,
                                                                   (uint32_t)limit, per_file, cos.data(), ids.data(), &count, &flag)
                        : cs_shards_search_variants_grouped(sh_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, per_file,
                                                            cos.data(), ids.data(), &count, &flag));
        else
            check(scope ? cs_index_search_variants_grouped_scoped(h_, scope->handle(), q.data(), (uint32_t)nq, (uint32_t)qdim,
                                                                  (uint32_t)limit, per_file, cos.data(), ids.data(), &count, &flag)
                        : cs_index_search_variants_grouped(h_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, per_file,
                                                           cos.data(), ids.data(), &count, &flag));
        if (high_confidence) *high_confidence = flag != 0;
        return results(cos, ids, count);
    }
    std::vector<SearchResult> search_variants(const std::vector<std::vector<float>>& variants, size_t limit,
                                              bool* high_confidence = nullptr) const {
        const size_t nq = variants.size();
        if (nq == 0) return {};
        const size_t qdim = variants[0].size();
        std::vector<float> q;
        for (const auto& v : variants) {
            if (v.size() != qdim) throw Error(CS_ERR_BAD_ARG, "queries of unequal length");
            q.insert(q.end(), v.begin(), v.end());
        }
        std::vector<float> cos(limit);
        std::vector<uint32_t> ids(limit);
        uint32_t count = 0;
        int32_t flag = 0;
        check(sh_ ? cs_shards_search_variants(sh_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, cos.data(),
                                              ids.data(), &count, &flag)
                  : cs_index_search_variants(h_, q.data(), (uint32_t)nq, (uint32_t)qdim, (uint32_t)limit, cos.data(),
                                             ids.data(), &count, &flag));
        if (high_confidence) *high_confidence = flag != 0;
        std::vector<SearchResult> out;
        for (uint32_t j = 0; j < count; ++j) {
            auto it = meta_.find(ids[j]);
            if (it == meta_.end()) continue;
            SearchResult r;
            r.id = ids[j];
            r.meta = it->second;
            r.distance = cs_cos_to_distance(cos[j]);
            r.score = 1.0f - r.distance;
            out.push_back(std::move(r));
        }
        return out;
    }
    std::optional<ChunkMetadata> get_chunk(uint32_t id) const {  // store.rs:709-713
        auto it = meta_.find(id);
        return it == meta_.end() ? std::nullopt : std::optional<ChunkMetadata>(it->second);
    }
    std::map<std::string, std::vector<uint32_t>> get_chunks_by_file() const {  // store.rs:529-543
        std::map<std::string, std::vector<uint32_t>> m;
        for (const auto& kv : meta_) m[kv.second.path].push_back(kv.first);
        return m;
    }
    StoreStats stats() const {  // store.rs:501-523
        StoreStats s;
        s.total_chunks = meta_.size();
        s.total_files = get_chunks_by_file().size();
        s.indexed = is_indexed();
        s.dimensions = dimensions_;
        s.max_chunk_id = meta_.empty() ? 0 : meta_.rbegin()->first;
        return s;
    }
    size_t dimensions() const { return dimensions_; }
    cs_index* handle() const { return h_; }
    // searches of >= n queries take the f16 filter + exact f32 refine path (default 2; 1 = always)
    void set_filter_min_queries(uint32_t n) { if (h_) check(cs_index_set_filter_min_queries(h_, n)); }
    void set_single_query_route(int32_t route) { if (h_) check(cs_index_set_single_query_route(h_, route)); }

  private:
    cs_index* h_ = nullptr;
    cs_shards* sh_ = nullptr;
    size_t dimensions_;
    bool grouped_ = true;  // a sharded store: whether it was opened with grouped = true
    void needs_groups() const {
        if (sh_ && !grouped_) throw Error(CS_ERR_UNSUPPORTED, "a sharded store has no grouped search unless it is opened with grouped = true");
    }
    uint32_t id_base_ = 0;
    std::map<uint32_t, ChunkMetadata> meta_;
};

// The tokenizer fastembed builds from the model's tokenizer.json (tokenizers 0.22.2): vocab.txt in,
// [CLS] ... [SEP] ids out (csrc/tokenizer.cpp).
class Tokenizer {
  public:
    explicit Tokenizer(const std::string& vocab_path, bool lowercase = true, uint32_t max_length = 512) {
        check(cs_tokenizer_create_from_file(vocab_path.c_str(), lowercase ? 1 : 0, max_length, &h_));
    }
    Tokenizer(const char* vocab_txt, size_t bytes, bool lowercase = true, uint32_t max_length = 512) {
        check(cs_tokenizer_create(vocab_txt, bytes, lowercase ? 1 : 0, max_length, &h_));
    }
    ~Tokenizer() { cs_tokenizer_destroy(h_); }
    Tokenizer(const Tokenizer&) = delete;
    Tokenizer& operator=(const Tokenizer&) = delete;

    // encode_batch: ids/mask [n, L] row-major, L = the batch's longest sequence
    size_t encode_batch(const std::vector<std::string>& texts, std::vector<int32_t>& ids, std::vector<int32_t>& mask,
                        uint32_t max_length = 0) const {
        std::string blob;
        std::vector<uint64_t> off;
        pack(texts, blob, off);
        uint32_t L = 0;
        check(cs_tokenizer_encode_batch(h_, blob.data(), off.data(), (uint32_t)texts.size(), max_length, nullptr,
                                        nullptr, 0, &L));
        ids.assign(texts.size() * L, 0);
        mask.assign(texts.size() * L, 0);
        if (!texts.empty())
            check(cs_tokenizer_encode_batch(h_, blob.data(), off.data(), (uint32_t)texts.size(), max_length,
                                            ids.data(), mask.data(), L, nullptr));
        return L;
    }
    int32_t token_to_id(const std::string& token) const { return cs_tokenizer_token_to_id(h_, token.c_str()); }
    size_t vocab_size() const { return cs_tokenizer_vocab_size(h_); }
    const cs_tokenizer* handle() const { return h_; }

    static void pack(const std::vector<std::string>& texts, std::string& blob, std::vector<uint64_t>& off) {
        off.assign(1, 0);
        for (const auto& t : texts) {
            blob += t;
            off.push_back(blob.size());
        }
    }

  private:
    cs_tokenizer* h_ = nullptr;
};

// FastEmbedder: from strings when a Tokenizer is attached (embed_batch(Vec<String>)), or from token ids.
class FastEmbedder {
  public:
    // with_cache_dir — embedder.rs:218-245; params == nullptr => synthetic weights from seed
    FastEmbedder(const cs_bert_config& cfg, const float* params, uint64_t seed = 0, int device = 0) {
        check(cs_embedder_create(&cfg, params, seed, device, &h_));
    }
    // with_cache_dir from a HF snapshot directory (config.json + model.safetensors)
    explicit FastEmbedder(const std::string& model_dir, cs_pooling pooling = CS_POOL_CLS, int device = 0) {
        check(cs_embedder_create_from_dir(model_dir.c_str(), (int32_t)pooling, device, &h_));
    }
    ~FastEmbedder() { cs_embedder_destroy(h_); }
    FastEmbedder(const FastEmbedder&) = delete;
    FastEmbedder& operator=(const FastEmbedder&) = delete;

    // embed_batch — embedder.rs:249-263 (batch 0 = CODESEARCH_BATCH_SIZE or 256/128/64)
    std::vector<std::vector<float>> embed_batch(const std::vector<int32_t>& ids, const std::vector<int32_t>& mask,
                                                size_t n, size_t seq_len,
                                                const volatile int32_t* shutdown = nullptr) {
        return embed_batch_chunked(ids, mask, n, seq_len, 0, shutdown);
    }
    // embed_batch_chunked — embedder.rs:266-295
    std::vector<std::vector<float>> embed_batch_chunked(const std::vector<int32_t>& ids,
                                                        const std::vector<int32_t>& mask, size_t n,
                                                        size_t seq_len, size_t batch_size,
                                                        const volatile int32_t* shutdown = nullptr) {
        const size_t d = dimensions();
        std::vector<float> flat(n * d);
        check(cs_embedder_embed_ids(h_, ids.data(), mask.data(), n, (uint32_t)seq_len, (uint32_t)batch_size,
                                    flat.data(), shutdown));
        std::vector<std::vector<float>> out(n);
        for (size_t i = 0; i < n; ++i) out[i].assign(flat.begin() + i * d, flat.begin() + (i + 1) * d);
        return out;
    }
    // embed_batch(texts) — embedder.rs:249-263, from strings
    void attach_tokenizer(const Tokenizer* t) { tok_ = t; }
    std::vector<std::vector<float>> embed_batch(const std::vector<std::string>& texts,
                                                const volatile int32_t* shutdown = nullptr) {
        return embed_batch_chunked(texts, 0, shutdown);
    }
    std::vector<std::vector<float>> embed_batch_chunked(const std::vector<std::string>& texts, size_t batch_size,
                                                        const volatile int32_t* shutdown = nullptr) {
        if (!tok_) throw Error(CS_ERR_UNSUPPORTED, "Failed to generate embeddings: no tokenizer attached");
        std::string blob;
        std::vector<uint64_t> off;
        Tokenizer::pack(texts, blob, off);
        const size_t d = dimensions(), n = texts.size();
        std::vector<float> flat(n * d);
        check(cs_embedder_embed_texts(h_, tok_->handle(), blob.data(), off.data(), n, (uint32_t)batch_size,
                                      flat.data(), shutdown));
        std::vector<std::vector<float>> out(n);
        for (size_t i = 0; i < n; ++i) out[i].assign(flat.begin() + i * d, flat.begin() + (i + 1) * d);
        return out;
    }
    // embed_one — embedder.rs:298-304
    std::vector<float> embed_one(const std::string& text) {
        auto r = embed_batch(std::vector<std::string>{text});
        if (r.empty()) throw Error(CS_ERR_BAD_ARG, "No embedding generated");
        return r[0];
    }
    // The reference's call shape on a queue (src/embed/batch.rs:84-115: slices of 32 under a mutex): submit() tokenises
    // and queues a slice, wait() returns its rows; the first wait embeds everything queued as full device batches.
    // Safe from several threads on one embedder.
    uint64_t submit(const std::vector<std::string>& texts) {
        if (!tok_) throw Error(CS_ERR_UNSUPPORTED, "Failed to generate embeddings: no tokenizer attached");
        std::string blob;
        std::vector<uint64_t> off;
        Tokenizer::pack(texts, blob, off);
        uint64_t ticket = 0;
        check(cs_embedder_submit_texts(h_, tok_->handle(), blob.data(), off.data(), texts.size(), &ticket));
        return ticket;
    }
    std::vector<std::vector<float>> wait(uint64_t ticket, size_t n, const volatile int32_t* shutdown = nullptr) {
        const size_t d = dimensions();
        std::vector<float> flat(n * d + 1);
        check(cs_embedder_wait(h_, ticket, flat.data(), shutdown));
        std::vector<std::vector<float>> out(n);
        for (size_t i = 0; i < n; ++i) out[i].assign(flat.begin() + i * d, flat.begin() + (i + 1) * d);
        return out;
    }
    void discard(uint64_t ticket) { check(cs_embedder_discard(h_, ticket)); }
    size_t dimensions() const { return cs_embedder_dim(h_); }  // embedder.rs:307
    cs_embedder* handle() const { return h_; }
    // CS_GEMM_SPLIT_F16 (default), CS_GEMM_F32 (exact-f32 MFMA) or, for a dynamically quantised model (a *Q registry
    // entry's directory: what it comes up in), CS_GEMM_Q8_DYNAMIC — include/codesearch_gpu.h
    void set_gemm_mode(cs_gemm_mode mode) { check(cs_embedder_set_gemm_mode(h_, (int32_t)mode)); }
    cs_gemm_mode gemm_mode() const { return (cs_gemm_mode)cs_embedder_gemm_mode(h_); }

  private:
    cs_embedder* h_ = nullptr;
    const Tokenizer* tok_ = nullptr;
};

// NeuralReranker — src/rerank/neural.rs:17-122: a cross-encoder scores every (query, document) pair on the device
// (cs_reranker_*); `rerank` orders by that score, `rerank_and_blend` blends its sigmoid with the min-max-normalised fusion
// scores, 0.575 / 0.425.  Built from a sequence-classification snapshot directory (config.json, model.safetensors,
// tokenizer.json or vocab.txt).
class NeuralReranker {
  public:
    static constexpr float RERANK_WEIGHT = 0.575f, RRF_WEIGHT = 0.425f;  // neural.rs:12-13
    explicit NeuralReranker(const std::string& model_dir, int device = 0, uint32_t max_length = 512) : max_length_(max_length) {
        check(cs_reranker_create_from_dir(model_dir.c_str(), device, &h_));
        const int32_t s = cs_tokenizer_create_from_dir(model_dir.c_str(), max_length, &tok_);
        if (s != CS_OK) { cs_reranker_destroy(h_); h_ = nullptr; check(s); }
    }
    ~NeuralReranker() { cs_tokenizer_destroy(tok_); cs_reranker_destroy(h_); }
    NeuralReranker(const NeuralReranker&) = delete;
    NeuralReranker& operator=(const NeuralReranker&) = delete;

    // (original index, rerank score), score descending — neural.rs:56-72
    std::vector<std::pair<size_t, float>> rerank(const std::string& query, const std::vector<std::string>& documents) {
        return run(query, documents, nullptr);
    }
    // (original index, blended score), descending — neural.rs:77-121
    std::vector<std::pair<size_t, float>> rerank_and_blend(const std::string& query, const std::vector<std::string>& documents,
                                                           const std::vector<float>& rrf_scores) {
        if (documents.size() != rrf_scores.size()) throw Error(CS_ERR_BAD_ARG, "Documents and RRF scores must have same length");
        return run(query, documents, rrf_scores.data());
    }
    cs_reranker* handle() const { return h_; }

  private:
    std::vector<std::pair<size_t, float>> run(const std::string& query, const std::vector<std::string>& documents, const float* rrf) {
        std::vector<std::pair<size_t, float>> out;
        if (documents.empty()) return out;  // neural.rs:57-59
        std::string blob;
        std::vector<uint64_t> off;
        Tokenizer::pack(documents, blob, off);
        std::vector<uint32_t> idx(documents.size());
        std::vector<float> score(documents.size());
        check(cs_reranker_rerank_texts(h_, tok_, query.c_str(), blob.data(), off.data(), documents.size(), max_length_, rrf, idx.data(),
                                       score.data()));
        for (size_t i = 0; i < idx.size(); ++i) out.emplace_back(idx[i], score[i]);
        return out;
    }
    cs_reranker* h_ = nullptr;
    cs_tokenizer* tok_ = nullptr;
    uint32_t max_length_ = 512;
};

// One encoder replica per GPU inside this process and the index loop of src/index/mod.rs:626-762 over a sharded
// VectorStore: every replica embeds the chunks whose ids fall on the shards of its own GPU, rows are appended without
// leaving HBM, no collective (cs_embedders_*).
class EmbedderReplicas {
  public:
    EmbedderReplicas(const cs_bert_config& cfg, const float* params, uint64_t seed, const std::vector<int32_t>& devices) {
        check(cs_embedders_create(&cfg, params, seed, devices.data(), (uint32_t)devices.size(), &h_));
    }
    EmbedderReplicas(const std::string& model_dir, cs_pooling pooling, const std::vector<int32_t>& devices) {
        check(cs_embedders_create_from_dir(model_dir.c_str(), (int32_t)pooling, devices.data(), (uint32_t)devices.size(), &h_));
    }
    ~EmbedderReplicas() { cs_embedders_destroy(h_); }
    EmbedderReplicas(const EmbedderReplicas&) = delete;
    EmbedderReplicas& operator=(const EmbedderReplicas&) = delete;
    void attach_tokenizer(const Tokenizer* t) { tok_ = t; }
    size_t dimensions() const { return cs_embedders_dim(h_); }
    size_t size() const { return cs_embedders_count(h_); }
    // embed_batch over all replicas: row i = text i
    std::vector<std::vector<float>> embed_batch(const std::vector<std::string>& texts, const volatile int32_t* shutdown = nullptr) {
        if (!tok_) throw Error(CS_ERR_UNSUPPORTED, "Failed to generate embeddings: no tokenizer attached");
        std::string blob;
        std::vector<uint64_t> off;
        Tokenizer::pack(texts, blob, off);
        const size_t d = dimensions(), n = texts.size();
        std::vector<float> flat(n * d + 1);
        check(cs_embedders_embed_texts(h_, tok_->handle(), blob.data(), off.data(), n, 0, flat.data(), shutdown));
        std::vector<std::vector<float>> out(n);
        for (size_t i = 0; i < n; ++i) out[i].assign(flat.begin() + i * d, flat.begin() + (i + 1) * d);
        return out;
    }
    // embed_chunks + insert_chunks_with_ids in one call on a SHARDED store -> the assigned ids (metadata: the caller's)
    std::vector<uint32_t> index_texts(cs_shards* store, const std::vector<std::string>& texts,
                                      const volatile int32_t* shutdown = nullptr) {
        if (!tok_) throw Error(CS_ERR_UNSUPPORTED, "Failed to generate embeddings: no tokenizer attached");
        std::string blob;
        std::vector<uint64_t> off;
        Tokenizer::pack(texts, blob, off);
        std::vector<uint32_t> ids(texts.size());
        check(cs_embedders_index_texts(h_, tok_->handle(), store, blob.data(), off.data(), texts.size(), 0, ids.data(), shutdown));
        return ids;
    }
    cs_embedders* handle() const { return h_; }

  private:
    cs_embedders* h_ = nullptr;
    const Tokenizer* tok_ = nullptr;
};

}  // namespace cs
