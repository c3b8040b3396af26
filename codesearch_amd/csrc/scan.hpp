// scan.hpp — launch interface of the cosine scan + top-k kernels (scan.hip).
#pragma once

#include "common.hpp"
#include "search_route.hpp"  // kFilterPhase0, kpad_for, prime_sample_rows

namespace cs {

struct ScanPlan {
    uint32_t blocks;     // scan grid.x
    uint32_t kpad;       // per-wave list capacity (power of two >= k, >= 64)
    uint32_t qtile;      // queries handled per scan pass
    uint32_t passes;     // ceil(nq / qtile)  (grid.y)
    bool deep;           // one block per CU with twice the rows in flight per wave (one query, k <= 64)
    size_t partial_keys; // u64 count needed for the scan's partial buffer
    size_t merge_keys;   // u64 count needed for the merge ping-pong buffer
};

// Geometry for a search of nq queries / top-k over n_rows rows of `dim` floats.
ScanPlan plan_scan(uint64_t n_rows, uint32_t dim, uint32_t nq, uint32_t k, int num_cus);

// Buffers of a primed scan (scan.hip, PRIME mode): a pass over a corpus prefix leaves in
// d_floor[q] a lower bound of query q's k-th best cosine, which the full scan starts from.
struct ScanPrime {
    float* d_wave_max = nullptr;  // [nq][4 * plan_prime().blocks]
    uint32_t* d_done = nullptr;   // [passes], zero between launches
    float* d_floor = nullptr;     // [nq]
};
bool scan_prime_supported(uint32_t dim);
ScanPlan plan_prime(uint64_t sample_rows, uint32_t dim, uint32_t nq, uint32_t k, int num_cus);

// Scores every live row of corpus[0..n_rows) against each query and leaves, per
// (query, block), the block's best k as packed keys in d_partial[q][block][k].
// prime + prime_pass: run the prime pass over these rows instead (plan from plan_prime, no
// partial lists written);  prime alone: start the lists from prime->d_floor.
int32_t launch_scan(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim,
                    const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead,
                    RowIds id_base, uint64_t* d_partial, hipStream_t stream,
                    const ScanPrime* prime = nullptr, bool prime_pass = false, const uint32_t* gate = nullptr);
// `gate` (launch_scan and launch_merge): device word; when non-null every block of the launch exits at
// once unless *gate != 0 — the exact rerun enqueued behind a batched search on the device API.

// Reduces nlists lists of k keys per query ([nq][nlists][k], or [nlists][nq][k] when
// list_major) to the best k per query,
// writing keys / decoded cosines / ids / counts (each optional).  d_tmp: ping-pong
// scratch of plan.merge_keys (may be null when nlists*k <= 2048).
int32_t launch_merge(const uint64_t* d_lists, uint32_t nlists, uint32_t nq, uint32_t k,
                     bool list_major, uint64_t* d_tmp_a, uint64_t* d_tmp_b, uint64_t* d_out_keys, float* d_out_cos,
                     uint32_t* d_out_ids, uint32_t* d_out_counts, hipStream_t stream,
                     const uint32_t* gate = nullptr, uint32_t remap_stripe = 0, uint32_t remap_shards = 0);
// remap_stripe != 0: list l holds shard l's local row numbers; they become global ids while the lists are
// read (striped row sharding, shards.hip).
size_t merge_tmp_keys(uint32_t nlists, uint32_t nq, uint32_t k);
// cs_merge_topk_device with the striped-shard id remap of launch_merge (index.hip; pooled scratch, asynchronous)
int32_t merge_topk_device_impl(int32_t device, const uint64_t* d_keys, uint32_t nlists, uint32_t nq, uint32_t k,
                               uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_counts,
                               hipStream_t stream, uint32_t remap_stripe, uint32_t remap_shards);

void merge_scratch_release(int device, hipStream_t stream);  // frees the pooled multi-level merge scratch of a stream
// shards.hip: make room for `rows` rows in all (the only step of an append that can run out of memory), and append
// rows resident on `src_device` with one asynchronous copy on `stream` (a stream of src_device).
int32_t index_reserve(cs_index* h, uint64_t rows);
int32_t index_append_from(cs_index* h, const float* d_rows, int src_device, uint64_t n, hipStream_t stream);

// Variant merge of search::search (src/search/mod.rs:513-611): keys [nv][k] -> the best `limit` distinct ids
// (a chunk keeps its best key), best-first, + count + the "top five all within distance 0.15" predicate.
int32_t launch_merge_variants(const uint64_t* d_keys, uint32_t nv, uint32_t k, uint32_t limit, uint64_t* d_out_keys,
                              float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_count,
                              uint32_t* d_out_high_confidence, hipStream_t stream);

// ---- masked search (scan_masked.hip, plan: masked_plan.hpp) ------------------------------------
// Row list of a masked search: the stored rows [0, n_rows) whose id lies in [allow_lo, allow_hi), has its bit set in
// d_allow (word w covers ids allow_lo + 32 w ...) and is not tombstoned, ascending, into d_list[0, list_cap);
// d_blocks[mask_list_blocks(n_rows) + 1] receives the per-block offsets and, last, the list length.
int32_t launch_mask_rows(const uint32_t* d_allow, uint64_t allow_lo, uint64_t allow_hi, const uint32_t* d_dead,
                         RowIds ids, uint64_t n_rows, uint32_t* d_blocks, uint32_t* d_list, uint64_t list_cap,
                         hipStream_t stream);
// The streaming scan over the rows d_list[0, *d_list_len) (plan: plan_scan of an upper bound of the length): the same
// per-block partial lists as launch_scan, for launch_merge.  prime + prime_pass: the prime pass over the first
// min(prime_rows, *d_list_len) entries (plan from plan_prime); prime alone: the lists start from prime->d_floor.
int32_t launch_scan_masked(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                           const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                           uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime = nullptr,
                           bool prime_pass = false, uint64_t prime_rows = 0);
// index.hip: a masked search of nq queries already in HBM (d_queries) enqueued on `stream` with the device-API scratch of
// (stream, calling thread); the best k per query as packed keys into d_out_keys [nq][k].  `allow` is host memory that must
// stay valid until the stream has passed the search.  Used by the sharded store.
int32_t index_search_masked_device(cs_index* h, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* allow,
                                   uint64_t allow_bits, uint64_t* d_out_keys, hipStream_t stream);
// index.hip: a grouped search (scan_grouped.hip) of nq queries already in HBM enqueued on `stream` with the same scratch,
// nothing waited for: the capped scan over every stored row (scope null) or the gathered capped scan over the scope's row
// list, then launch_merge_grouped; the capped best k per query as packed keys into d_out_keys [nq][k], zeros behind the
// count.  Where the host form returns the empty answer without a launch (a scope with no live row, an index with no stored
// row) the slot is zeroed on the stream instead.  A scope counts the call in its gathered_searches; it is refreshed first
// when that is due (which waits for the device, as cs_index_search_scoped_device does).  Used by the sharded store.
int32_t index_search_grouped_device(cs_index* h, cs_scope* scope, const float* d_queries, uint32_t nq, uint32_t k,
                                    uint32_t per_group, uint64_t* d_out_keys, hipStream_t stream);

// ---- scopes (index.hip cs_scope; plan: masked_plan.hpp) ------------------------------------------
// Row list of a scope: for the strictly ascending chunk ids d_scope_ids[0, n_ids), the stored rows [0, n_rows) that hold
// them and are not tombstoned, ascending, into d_list[0, list_cap); d_blocks[scope_list_blocks(n_ids) + 1] receives
// the per-block offsets and, last, the list length.  Work and launches follow n_ids, not n_rows.
int32_t launch_scope_rows(const uint32_t* d_scope_ids, uint64_t n_ids, const uint32_t* d_dead, RowIds ids, uint64_t n_rows,
                          uint32_t* d_blocks, uint32_t* d_list, uint64_t list_cap, hipStream_t stream);
// What a scope that can take the int8 filter keeps beside its list (scoped_filter_plan.hpp), from d_list[0, *d_len),
// *d_len <= list_cap: d_blocked[scope_blocked_words(n_rows)] = one bit per stored row, 1 where the row is NOT in the list (the
// list holds live rows only, so tombstoned rows are blocked too; bits past n_rows are 1), and d_table[0] = the last
// entry, d_table[1 + j] = d_list[1024 j] (1 + ceil(list_cap / 1024) words).
int32_t launch_scope_filter_state(const uint32_t* d_list, const uint32_t* d_len, uint64_t list_cap, uint64_t n_rows,
                                  uint32_t* d_blocked, uint32_t* d_table, hipStream_t stream);
// index.hip, for the sharded store: the live rows of a scope of h after the refresh that is due, if one is
// (scope_refresh_due); the index must be built.
int32_t index_scope_live_rows(cs_index* h, cs_scope* scope, uint64_t* live_rows);

// ---- scope algebra (scope_ops.hip; plan: scope_ops_plan.hpp) ---------------------------------------
// scan_masked.hip: d_blocks[0, nb) -> their exclusive prefix sums, d_blocks[nb] = the total (mask_scan_kernel, one block).
int32_t launch_mask_scan(uint32_t* d_blocks, uint32_t nb, hipStream_t stream);
// The set operation `op` (CS_SCOPE_OP_*) over the strictly ascending d_a[0, na) and d_b[0, nb).  Count: d_tiles
// [scope_ops_tiles(na, nb) + 1] receives the per-tile offsets of the result and, last, its length (mod 2^32).  Write: the
// result, ascending, into d_out[0, out_cap) from the offsets the count pass left.
int32_t launch_scope_ops_count(const uint32_t* d_a, uint64_t na, const uint32_t* d_b, uint64_t nb, int32_t op, uint32_t* d_tiles,
                               hipStream_t stream);
int32_t launch_scope_ops_write(const uint32_t* d_a, uint64_t na, const uint32_t* d_b, uint64_t nb, int32_t op, uint32_t* d_tiles,
                               uint32_t* d_out, uint64_t out_cap, hipStream_t stream);
// d_out[i] = first + i for i < n (first + n <= 2^32).
int32_t launch_scope_range(uint32_t first, uint64_t n, uint32_t* d_out, hipStream_t stream);
// shards.hip: positions [first, first + n) of a sharded scope's global ids, ascending (the parts' ids read back, restated
// as global ids and merged on the host); the range has been checked.
int32_t shards_scope_read_ids(const cs_scope* scope, uint64_t first, uint64_t n, uint32_t* out_ids);

// ---- grouped search (scan_grouped.hip, plan: grouped_plan.hpp) -----------------------------------
// The group table of an index as the kernels read it: groups[id - id_base] for ids below id_base + len, CS_NO_GROUP for
// every other id (and for all of them when groups is null); at most per_group rows of a group are kept.
struct GroupView {
    const uint32_t* groups = nullptr;
    uint32_t len = 0;
    uint32_t id_base = 0;
    uint32_t per_group = 0xFFFFFFFFu;
};
struct GroupedPlan;
// The streaming scan's arithmetic with capped per-wave lists: d_partial[q][plan.lists][k], one unsorted list per wave.
int32_t launch_scan_grouped(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim,
                            const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids,
                            const GroupView& gv, uint64_t* d_partial, hipStream_t stream);
// Those lists -> the capped best k per query; every level caps.  Outputs as launch_merge's (each optional); d_tmp_a / d_tmp_b:
// plan.merge_keys keys each (may be null when plan.merge_levels == 1).
int32_t launch_merge_grouped(const GroupedPlan& plan, const uint64_t* d_lists, uint32_t nq, uint32_t k, const GroupView& gv,
                             uint64_t* d_tmp_a, uint64_t* d_tmp_b, uint64_t* d_out_keys, float* d_out_cos,
                             uint32_t* d_out_ids, uint32_t* d_out_counts, hipStream_t stream);

// launch_scan_grouped over the live rows d_list[0, *d_list_len) (a scope's row list, ascending; plan: plan_grouped of the
// length): the same per-wave capped lists, for launch_merge_grouped.  The list holds live rows only: no tombstone test.
int32_t launch_scan_grouped_list(const GroupedPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const GroupView& gv, uint64_t* d_partial, hipStream_t stream);
// launch_merge_variants under the cap: capped per-variant lists d_keys [nv][k] -> the capped best k distinct ids (a chunk
// keeps its best key), best first, + count + the high-confidence predicate on the list returned.  Every level
// de-duplicates and caps (grouped_plan.hpp); d_tmp_a / d_tmp_b: grouped_variants_tmp_keys(nv, k) keys each (may be null
// when that is 0).
int32_t launch_merge_variants_grouped(const uint64_t* d_keys, uint32_t nv, uint32_t k, const GroupView& gv, uint64_t* d_tmp_a,
                                      uint64_t* d_tmp_b, uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                                      uint32_t* d_out_count, uint32_t* d_out_high_confidence, hipStream_t stream);

// ---- grouped search over a sharded store (scan_shards_grouped.hip, plan: shards_grouped_plan.hpp) ---------
struct ShardsGroupedPlan;
// The root's capped shard merge: d_gathered = [nshards][nq][k] capped lists of (cosine, local row) keys -> the capped best
// k per query as global keys in d_out_keys [nq][k] (may be pinned host memory), under gv = the root's table by global id.
// d_first: plan.first_keys keys, d_tmp_a / d_tmp_b: plan.merge_keys keys each (each may be null when that is 0).
int32_t launch_merge_shards_grouped(const ShardsGroupedPlan& plan, const uint64_t* d_gathered, uint32_t nshards, uint32_t nq,
                                    uint32_t k, uint32_t stripe, const GroupView& gv, uint64_t* d_first, uint64_t* d_tmp_a,
                                    uint64_t* d_tmp_b, uint64_t* d_out_keys, hipStream_t stream);

// ---- similar-chunk search (scan_similar.hip, sources: similar_sources.hpp) -------------------------------
// What a similar-chunk search may not return, per query, and its bound: query q never gets the row whose id is
// d_ex_ids[q] (an id no row carries: nothing) nor a row whose group is d_ex_groups[q] (CS_NO_GROUP: nothing); only rows
// with cosine > min_cos are kept (-inf: all; never NaN).
struct SimilarView {
    const uint32_t* d_ex_ids = nullptr;     // [nq]
    const uint32_t* d_ex_groups = nullptr;  // [nq]
    float min_cos = -__builtin_huge_valf();
};
// d_queries[q] = the stored row d_rows[q] of d_corpus, verbatim, for q < nq (every d_rows[q] a stored row).
int32_t launch_gather_sources(const float* d_corpus, uint32_t dim, const uint32_t* d_rows, uint32_t nq, float* d_queries,
                              hipStream_t stream);
// The streaming scan's arithmetic under those exclusions (plan: plan_scan): the same per-block partial lists as
// launch_scan, for launch_merge.  gv.per_group is not read.
int32_t launch_scan_similar(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries,
                            uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const GroupView& gv,
                            const SimilarView& sv, uint64_t* d_partial, hipStream_t stream);
// launch_scan_similar over the live rows d_list[0, *d_list_len) (a scope's row list, ascending; plan: plan_scan of the
// length): the gathered scan's arithmetic under those exclusions, the same per-block partial lists, for launch_merge.  The
// list holds live rows only: no tombstone test.
int32_t launch_scan_similar_list(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const GroupView& gv, const SimilarView& sv, uint64_t* d_partial, hipStream_t stream);

// The similar-chunk search through the filter (scan_similar_filter.hip): what launch_scan_split needs to hand every phase's
// candidates to the similar refine and fold instead of the ordinary ones.
struct SimilarRefine {
    SimilarView sv;
    GroupView gv;  // per_group is not read
};
struct BatchedState;
struct SplitQueryWs;
// rescore_keys_kernel's work and grid (rk_blocks blocks per query; first_rows != 0: phase 0, candidate i is row i) with the
// similar search's final store: the key is empty unless the cosine is > sv.min_cos and the query keeps the row.
// d_list != null with first_rows != 0 (phase 0 of a scoped call): candidate i is row d_list[i], i < first_rows <= cap, and
// no bitmap is read — the list holds live, allowed rows only.
int32_t launch_similar_rescore(const BatchedState& st, const SplitQueryWs& qw, const float* d_corpus, uint32_t dim,
                               const float* d_queries, uint32_t nq, uint32_t cap, uint32_t rk_blocks, uint32_t first_rows,
                               const uint32_t* d_dead, RowIds ids, const GroupView& gv, const SimilarView& sv,
                               hipStream_t stream, const uint32_t* d_list = nullptr);
// launch_select_candidates whose threshold never falls below sv.min_cos.
int32_t launch_similar_select(const BatchedState& st, uint32_t nq, uint32_t cap, uint32_t k, bool last, const SimilarView& sv,
                              uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_counts,
                              hipStream_t stream);

// ---- boosted search (scan_boosted.hip; plan: plan_scan) ---------------------------------------------------
// What a boosted search weighs rows by: the class table of the index as the kernels read it — classes[id - id_base] for
// ids below id_base + len, no class for every other id (and for all of them when classes is null) — and the call's own
// weight table on the device.  A row weighs weights[class] when its class is below n_classes, else 1.  wmin / wmax: the
// smallest and the largest weight a row can take (the table's extremes, widened to hold 1).
struct BoostView {
    const uint16_t* classes = nullptr;
    uint32_t len = 0;
    uint32_t id_base = 0;
    const float* weights = nullptr;  // [n_classes]
    uint32_t n_classes = 0;
    float wmin = 1.0f, wmax = 1.0f;
};
// The streaming scan's arithmetic selecting by b = fl(score(cosine) * weight): the same per-block partial lists as
// launch_scan, holding packed keys of (b, id), for launch_merge.
// prime + prime_pass: the prime pass over these rows instead (plan from plan_prime, tuned dims only, no partial lists
// written): d_floor[q] = a lower bound of query q's k-th best b;  prime alone: the lists start from prime->d_floor.
int32_t launch_scan_boosted(const ScanPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries,
                            uint32_t nq, uint32_t k, const uint32_t* d_dead, RowIds ids, const BoostView& bv,
                            uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime = nullptr, bool prime_pass = false);
// launch_scan_boosted over the live rows d_list[0, *d_list_len) (a scope's row list, ascending; plan: plan_scan of the
// length).  The list holds live rows only: no tombstone test.  A prime pass takes the first min(prime_rows, *d_list_len)
// entries.
int32_t launch_scan_boosted_list(const ScanPlan& plan, const float* d_corpus, uint32_t dim, const uint32_t* d_list,
                                 const uint32_t* d_list_len, const float* d_queries, uint32_t nq, uint32_t k, RowIds ids,
                                 const BoostView& bv, uint64_t* d_partial, hipStream_t stream, const ScanPrime* prime = nullptr,
                                 bool prime_pass = false, uint64_t prime_rows = 0);
// The merged winners d_keys [nq][k] (every non-empty key names a stored row of [0, n_rows), n_rows > 0) -> out_cos[nq][k] =
// the streaming scan's cosine of each winner's row, 0 for an empty slot; out_keys (optional) receives the keys as they are.
int32_t launch_boosted_cos(const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nq, uint32_t k,
                           RowIds ids, const uint64_t* d_keys, uint64_t* out_keys, float* out_cos, hipStream_t stream);

// ---- boosted search under the per-file cap, and across query variants (scan_boosted_grouped.hip; plan: plan_grouped) ----
// launch_scan_boosted's selection by b with launch_scan_grouped's capped per-wave lists: d_partial[q][plan.lists][k], one
// unsorted capped list of packed (b, id) keys per wave, for launch_merge_grouped.  No prime pass.  d_list / d_list_len null:
// every stored row [0, n_rows) with the tombstone test; else the live rows d_list[0, *d_list_len) (a scope's row list,
// ascending; the plan made for its length), and n_rows / d_dead are not read.
int32_t launch_scan_boosted_grouped(const GroupedPlan& plan, const float* d_corpus, uint64_t n_rows, uint32_t dim,
                                    const uint32_t* d_list, const uint32_t* d_list_len, const float* d_queries, uint32_t nq,
                                    uint32_t k, const uint32_t* d_dead, RowIds ids, const BoostView& bv, const GroupView& gv,
                                    uint64_t* d_partial, hipStream_t stream);
// launch_boosted_cos for the ONE merged list d_keys[k] of nv query variants: out_cos[j] = the largest of winner j's
// cosines over the variants (each the streaming scan's, bit for bit), 0 for an empty slot; out_keys as there.
int32_t launch_boosted_variants_cos(const float* d_corpus, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nv,
                                    uint32_t k, RowIds ids, const uint64_t* d_keys, uint64_t* out_keys, float* out_cos,
                                    hipStream_t stream);

// ---- similar-pairs search (scan_pairs.hip, plan: pairs_plan.hpp) -----------------------------------------
// A qualifying pair as the refine leaves it: the cosine's bits, the lower id, the higher id.
struct PairRecord {
    float cos;
    uint32_t a, b;
    uint32_t pad;
};
// The self-join's filter over the tile pairs [band_first, band_first + band_count) of the upper triangle of `tiles` x `tiles`
// 128-row tiles of d_split (the tiled f16 unit copy): every pair of stored rows rowA < rowB, both below n_rows, neither
// tombstoned (d_dead may be null), not of one group when other_group, whose f16 product is not <= min_cos - margin is
// appended as (rowA | rowB << 32) to d_cand[0, cand_cap).  *d_cnt (64 bits: a band can hold more than 2^32 pairs) keeps
// counting past cand_cap and stores stop at it; once it is past cand_cap, blocks that have not started yet score nothing.
int32_t launch_pairs_filter(const _Float16* d_split, uint32_t dim, uint64_t tiles, uint64_t band_first, uint64_t band_count,
                            uint64_t n_rows, const uint32_t* d_dead, RowIds ids, const GroupView& gv, bool other_group,
                            float min_cos, float margin, uint64_t* d_cand, uint64_t* d_cnt,
                            uint32_t cand_cap, hipStream_t stream);
// Every candidate d_cand[0, n) re-scored from the f32 corpus with the streaming scan's arithmetic, the lower id's row as
// the query; those with a finite cosine > min_cos become records d_out[0, *d_total) in no particular order (*d_total is
// zeroed by the caller).
int32_t launch_pairs_rescore(const float* d_corpus, uint32_t dim, const uint64_t* d_cand, uint32_t n, RowIds ids, float min_cos,
                             PairRecord* d_out, uint32_t* d_total, uint32_t blocks, hipStream_t stream);

// ---- scoped similar-pairs search (scan_pairs_scoped.hip, plan: pairs_scoped_plan.hpp) ----------------------
// Packed row i of d_packed (ceil(n_list / 128) whole tiles of the filter copy's tiled layout) = the unit row of stored row
// d_list[i] rounded to f16, from the f32 row and d_norms with launch_corpus_split's arithmetic; packed rows past n_list
// are zeros.
int32_t launch_pairs_pack(const float* d_corpus, const float* d_norms, const uint32_t* d_list, uint64_t n_list, uint32_t dim,
                          _Float16* d_packed, hipStream_t stream);
struct PairsScopedPlan;
// launch_pairs_filter over the tile pairs [band_first, band_first + band_count) of the plan's triangle (one packed buffer
// and list, passed twice) or rectangle (two): candidates are appended as stored rows (lower | higher << 32) through the
// lists (ascending live rows; plan.rows_a / rows_b of them), each unordered pair once however the lists overlap.  The
// counter and the cap (plan.cand_cap) as there.
int32_t launch_pairs_scoped_filter(const PairsScopedPlan& plan, const _Float16* d_packed_a, const _Float16* d_packed_b,
                                   const uint32_t* d_list_a, const uint32_t* d_list_b, uint32_t dim, uint64_t band_first,
                                   uint64_t band_count, RowIds ids, const GroupView& gv, bool other_group, float min_cos,
                                   float margin, uint64_t* d_cand, uint64_t* d_cnt, hipStream_t stream);

// ---- similar-clusters search (scan_clusters.hip, plan: clusters_plan.hpp) ----------------------------------
// d_parent[r] = r and d_mark[r] = 0 for the stored rows: every row its own component.
int32_t launch_clusters_init(uint32_t* d_parent, uint32_t* d_mark, uint64_t n_rows, hipStream_t stream);
// d_tile_root[t] = the common root of the live rows of tile t (128 rows), kClustersNoRoot when they have none,
// kClustersEmptyTile when no row of the tile is live.
int32_t launch_clusters_tile_roots(uint32_t* d_parent, uint64_t tiles, uint64_t n_rows, const uint32_t* d_dead,
                                   uint32_t* d_tile_root, hipStream_t stream);
// launch_pairs_filter's join over the tile pairs [first, first + count), into the union-find d_parent: a tile pair whose
// tiles share a root in d_tile_root (or with an empty tile) is skipped and counted in d_counters[1]; a pair of stored, live,
// non-excluded rows with a product above min_cos + margin (finite, both norms of ordinary size; d_norms null: never) is
// united at once; one not <= min_cos - margin otherwise is appended to d_amb[0, amb_cap) and counted in d_counters[0], which
// keeps counting past amb_cap (the launch is then void: blocks that have not started score nothing).
int32_t launch_clusters_join(const _Float16* d_split, uint32_t dim, uint64_t tiles, uint64_t first, uint64_t count,
                             uint64_t n_rows, const uint32_t* d_dead, RowIds ids, const GroupView& gv, bool other_group,
                             float min_cos, float margin, const float* d_norms, uint32_t* d_parent,
                             const uint32_t* d_tile_root, uint64_t* d_amb, uint64_t* d_counters, uint32_t amb_cap,
                             hipStream_t stream);
// Every pair d_amb[0, n) re-scored as launch_pairs_rescore does and united when its cosine is finite and > min_cos.
int32_t launch_clusters_rescore(const float* d_corpus, uint32_t dim, const uint64_t* d_amb, uint32_t n, RowIds ids, float min_cos,
                                uint32_t* d_parent, uint32_t blocks, hipStream_t stream);
// d_label[id - ids.base] = the id of the root of the id's row, for every live row (other slots are left alone: the caller
// fills them); d_parent is flattened; d_totals[0] += components of two or more rows, d_totals[1] += rows in them.
int32_t launch_clusters_label(uint32_t* d_parent, uint32_t* d_mark, uint64_t n_rows, const uint32_t* d_dead, RowIds ids,
                              uint32_t* d_label, uint64_t n_labels, uint64_t* d_totals, hipStream_t stream);

// ---- scoped similar-clusters search (scan_clusters_scoped.hip, plan: clusters_scoped_plan.hpp) --------------
// The union-find stays over stored rows (d_parent, d_mark: [stored rows]), but only the words of the rows the two lists
// name (ascending live rows; rows_b == 0: one list) are written or read by anything below.
// d_parent[r] = r and d_mark[r] = 0 for every row of the lists.
int32_t launch_clusters_scoped_init(uint32_t* d_parent, uint32_t* d_mark, const uint32_t* d_list_a, uint64_t rows_a,
                                    const uint32_t* d_list_b, uint64_t rows_b, hipStream_t stream);
// d_tile_root[t] = the common root of the rows of packed tile t of the list (entries [128 t, 128 t + 128) below `rows`),
// kClustersNoRoot when they have none; ceil(rows / 128) words.
int32_t launch_clusters_scoped_tile_roots(uint32_t* d_parent, const uint32_t* d_list, uint64_t rows, uint32_t* d_tile_root,
                                          hipStream_t stream);
struct ClustersScopedPlan;
// launch_clusters_join over the tile pairs [first, first + count) of the plan's triangle (one packed buffer, list and root
// array, passed twice) or rectangle (two), packed as launch_pairs_pack leaves them: pairs are united, or appended to
// d_amb[0, plan.ambiguous_cap) as stored rows (lower | higher << 32), through the lists; a row that meets itself is no pair.
// The counters as there.  d_norms is required.
int32_t launch_clusters_scoped_join(const ClustersScopedPlan& plan, const _Float16* d_packed_a, const _Float16* d_packed_b,
                                    const uint32_t* d_list_a, const uint32_t* d_list_b, uint32_t dim, uint64_t first,
                                    uint64_t count, RowIds ids, const GroupView& gv, bool other_group, float min_cos,
                                    float margin, const float* d_norms, uint32_t* d_parent, const uint32_t* d_root_a,
                                    const uint32_t* d_root_b, uint64_t* d_amb, uint64_t* d_counters, hipStream_t stream);
// Entry i of the two lists laid end to end: d_out_ids[i] = its id, d_out_label[i] = the id of its row's root (rows_a + rows_b
// words each); d_parent is flattened; d_totals[0] += components of two or more rows, d_totals[1] += rows in them, a row in
// both lists counted once.
int32_t launch_clusters_scoped_label(uint32_t* d_parent, uint32_t* d_mark, const uint32_t* d_list_a, uint64_t rows_a,
                                     const uint32_t* d_list_b, uint64_t rows_b, RowIds ids, uint32_t* d_out_ids,
                                     uint32_t* d_out_label, uint64_t* d_totals, hipStream_t stream);

// corpus[(first_out_row + r) * dim + c] = cs_synth_value(seed, (first_row + r) * dim + c)
int32_t launch_synth_fill(float* d_rows, uint64_t n, uint32_t dim, uint64_t seed,
                          uint64_t first_row, hipStream_t stream);

// ---- batched-query (MFMA) path, scan_mfma.hip ---------------------------------------------
// Candidate counters sit one per 128-byte line: appends are device-scope atomics, and ops on one
// line serialise at ~40 ns apiece whichever word they hit (measured: nine queries' counters in one
// line made the k=200 filter phases 50-190 us longer).
constexpr uint32_t kCntStride = 32;
// Device-API searches of up to this many queries carry a gated exact rerun behind the filter path (index.hip
// run_search); above it an overflowed candidate buffer is reported through the sticky word of BatchedState.
constexpr uint32_t kGatedMaxQ = 16;
// The fold's block and the keys it sorts per chunk (scan_mfma.hip MB_SEL_THREADS / MB_SEL_CAP; scan_similar_filter.hip
// restates the kernel)
constexpr uint32_t kSelThreads = 1024, kSelCap = 4096;
struct BatchedState {
    uint64_t* d_cand = nullptr;   // [nq][cap] candidate keys
    uint32_t* d_cnt = nullptr;    // [nq][kCntStride], word 0 of each line used
    float* d_tau = nullptr;       // [nq]
    uint64_t* d_carry = nullptr;  // [nq][k]
    // [0] = a candidate buffer overflowed during the current search (reset by the search's first kernel);
    // [1] = sticky: set with [0], cleared only by cs_index_search_status; [2] = overflowed searches counted so far
    // (the first kernel of the NEXT search folds [0] into it)
    uint32_t* d_overflow = nullptr;
    // pinned host word the first kernel of every search copies [2] into: lets the host notice overflowed device-API
    // searches (which it never waits for) a search or two later, without a synchronisation (index.hip: int8 strikes)
    uint32_t* h_mirror = nullptr;
};
// One block per query folds st.d_cand[q][0..cnt[q]) (packed keys) into st.d_carry[q][k], sets
// tau[q] to the k-th best cosine and resets cnt[q]; with `last` it also writes the outputs.
int32_t launch_select_candidates(const BatchedState& st, uint32_t nq, uint32_t cap, uint32_t k, bool last,
                                 uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                                 uint32_t* d_out_counts, hipStream_t stream);
bool batched_supported(uint32_t dim);
uint32_t batched_cap(uint32_t k);
int32_t launch_row_norms(const float* d_corpus, uint64_t first, uint64_t n, uint32_t dim,
                         float* d_norms, hipStream_t stream);
// Exact unless *st.d_overflow != 0 afterwards (then rerun on the list-based scan).
int32_t launch_scan_batched(const BatchedState& st, const float* d_corpus, const float* d_norms,
                            uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nq, uint32_t k,
                            const uint32_t* d_dead, RowIds id_base, int num_cus, uint64_t* d_out_keys,
                            float* d_out_cos, uint32_t* d_out_ids, uint32_t* d_out_counts,
                            hipStream_t stream);

// ---- batched-query filter-and-refine path (f16 unit-vector filter + exact refine), scan_filter.hip
struct SplitQueryWs {
    _Float16* d_qsplit = nullptr;  // [nq][dim] f16: q / |q|
    float* d_qmag = nullptr;       // [nq]
    // Host-buffer searches: the queries still sit in pinned host memory (device-addressable) and
    // d_queries is an empty device buffer — the prep kernel reads them from here and fills it,
    // which saves the H2D copy call (~6 us of a 45-us search over a small corpus).  Null otherwise.
    const float* q_pinned = nullptr;
    int8_t* d_q8q = nullptr;       // [nq][dim] int8: q / |q| on the query's own scale (int8 filter copy)
    float4* d_qmeta = nullptr;     // [4 nq]: [q] = {127 / max |q_i / |q||, 0.5001 sum |b_i|, q / |q| . mu, sqrt(sum b_i^2)},
                                   // [nq + q].x = sqrt(sum d_i^2), d = the query's rounding errors (q8_threshold);
                                   // [2 nq + q], [3 nq + q]: the same for the two-plane (128 times finer) quantisation
    int8_t* d_q8q_hi = nullptr;    // [nq][dim] x 2: the query as 128 hi + lo, both int8 (up to 64 queries)
    int8_t* d_q8q_lo = nullptr;
};
// int8 filter copy of the corpus (scan_filter.hip, "int8 filter copy"): complete 128-row tiles [0, rows / 128)
struct Q8View {
    const int8_t* d_q8 = nullptr;    // [tile][dim / 128][128 rows][128 B]
    const float4* d_tmeta = nullptr; // [tile] {127 / max |u - mu|, 0.5001 max row sum |a_i|, max row error norm, max row norm of a};
                                     // x = NaN: every row is a candidate
    const float* d_mu = nullptr;     // [dim] the mean unit row the copy is centred on (q.u = q.(u - mu) + q.mu)
    uint64_t rows = 0;               // multiple of 128
};
bool split_scan_supported(uint32_t dim);
// rows [first_tile * 128, (first_tile + ntiles) * 128) of the f32 corpus -> int8 tiles + their scales
int32_t launch_corpus_q8(const float* d_corpus, const float* d_norms, int8_t* d_q8, float4* d_tmeta, uint64_t first_tile,
                         uint64_t ntiles, uint32_t dim, const float* d_mu, hipStream_t stream);
// d_mu[dim] = mean over rows [0, n) of x / |x|
int32_t launch_unit_mean(const float* d_corpus, const float* d_norms, uint64_t n, uint32_t dim, float* d_mu,
                         hipStream_t stream);
// rows [first, first+n) of the f32 corpus, divided by their norms, as f16 -> the filter copy
// [rows][dim] (same row order; half the bytes of the f32 matrix)
int32_t launch_corpus_split(const float* d_corpus, const float* d_norms, _Float16* d_split, uint64_t first,
                            uint64_t n, uint32_t dim, hipStream_t stream);
// Exact (bit-identical to launch_scan + launch_merge) unless *st.d_overflow != 0 afterwards.
int32_t launch_scan_split(const BatchedState& st, const SplitQueryWs& qw, const float* d_corpus,
                          const _Float16* d_split, uint64_t n_rows, uint32_t dim, const float* d_queries, uint32_t nq, uint32_t k, const uint32_t* d_dead,
                          RowIds id_base, uint64_t* d_out_keys, float* d_out_cos, uint32_t* d_out_ids,
                          uint32_t* d_out_counts, hipStream_t stream, float margin, const Q8View* q8 = nullptr,
                          const FilterPlan* prepared = nullptr, const uint32_t* d_phase0_list = nullptr,
                          const SimilarRefine* similar = nullptr);
// What one phase's filter launch reads and writes beside the phase itself: the search state (tau, the counters and the
// candidate slots), the query workspace prep_queries_kernel filled, the two corpus copies and the tombstones.
struct FilterOperands {
    const BatchedState* st = nullptr;
    const SplitQueryWs* qw = nullptr;
    const _Float16* d_split = nullptr;  // the f16 kernels' operand
    const Q8View* q8 = nullptr;         // the int8 kernels' operand
    const uint32_t* d_dead = nullptr;   // may be null
    uint32_t nq = 0, cap = 0;           // cap: candidate slots per query
    float margin = 0.0f;                // filter_margin (the f16 kernels)
    uint32_t nt_stream = 1;             // FilterKnobs::nt
    hipStream_t stream = nullptr;
};
// The first kernel of a filter search (prep_queries_kernel): magnitudes, the f16 unit queries, with use_q8 the int8 plane and
// its constants against d_mu (with two_planes the hi / lo planes too), and the search state reset — tau = -inf, every
// counter = first_rows, the carried keys zeroed.
int32_t launch_prep_queries(uint32_t dim, const BatchedState& st, const SplitQueryWs& qw, const float* d_queries, uint32_t nq,
                            uint32_t k, uint32_t first_rows, const float* d_mu, bool use_q8, bool two_planes, hipStream_t stream);
// One phase as planned (filter_plan.hpp): the filter kernel ph.kernel / ph.nqt over rows [ph.lo, ph.filter_hi) (f16: ph.hi)
// on ph.grid blocks, then tail_candidates_kernel over [ph.tail_lo, ph.tail_hi).  launch_scan_split calls it per phase;
// cs_debug_filter (diagnostics.hip) calls it alone.  CS_ERR_BAD_ARG: a (kernel, nqt) that was never instantiated for this
// dim, rows that are not whole tiles where the kernel needs them, a resident-query grid off the XCD octets or below one
// octet per query tile, a missing operand.
int32_t launch_filter_phase(uint32_t dim, const FilterPhase& ph, const FilterOperands& op);
const FilterKnobs& filter_knobs();  // the plan's laboratory knobs as the launcher reads them (the product: the defaults)
// prepared (a scoped search, scoped_filter_plan.hpp): launch that plan instead of plan_filter's — its phase 0 re-scores
// the first prepared->phase0_rows entries of d_phase0_list, and d_dead is the scope's blocked-rows bitmap.
// similar (a similar-chunk search, scan_similar_filter.hip): every phase's refine and fold are the similar ones; not with a
// prepared plan.
// Proven bound of |filter cosine - exact cosine| for unit vectors of this width (scan_filter.hip header);
// `subnormals_exact` = the f16 MFMA consumes subnormal inputs exactly (sh_denorm_selftest).
float filter_margin(uint32_t dim, bool subnormals_exact);
int32_t sh_denorm_selftest(bool* ok, hipStream_t s);  // gemm_split.hip

}  // namespace cs
