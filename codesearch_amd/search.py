"""Host-side mirror of the step right after the scan in `search::search`
(/root/reference/src/search/mod.rs:494-611): retrieval limit, the cross-variant merge
(dedup by id keeping the best score, top retrieval_limit, score-descending) and the
early-termination predicate.  Rank arithmetic on <= 9 x 200 items — host work by design."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

from .vector_store import NO_GROUP, Scope, SearchResult

HIGH_CONFIDENCE_THRESHOLD = 0.15  # mod.rs:598: distance < 0.15 (cos > 0.7 under arroy's Cosine)
EARLY_TERMINATION_TOP_N = 5       # mod.rs:599


def retrieval_limit(max_results: int, vector_only: bool, is_identifier_query: bool) -> int:
    """mod.rs:494-502."""
    if vector_only:
        return max_results
    if is_identifier_query:
        return max(max_results * 3, 100)
    return max(max_results * 5, 200)


def merge_variant_results(per_variant: Sequence[Sequence[SearchResult]], limit: int) -> List[SearchResult]:
    """mod.rs:513-590: keep, per chunk id, the result with the highest score across query
    variants; take the `limit` best; sort by score descending."""
    best = {}
    for results in per_variant:
        for r in results:
            cur = best.get(r.id)
            if cur is None or r.score > cur.score:
                best[r.id] = r
    merged = sorted(best.values(), key=lambda r: -r.score)[:limit]
    return merged


def _trim_start(s: str, p: str) -> str:
    while p and s.startswith(p):  # Rust's trim_start_matches: every repetition
        s = s[len(p):]
    return s


def _trim_end(s: str, p: str) -> str:
    while p and s.endswith(p):
        s = s[:-len(p)]
    return s


def normalize_path_str(path: str) -> str:
    """src/cache/file_meta.rs:23-25: the UNC prefix stripped, backslashes as forward slashes."""
    return _trim_start(path, "\\\\?\\").replace("\\", "/")


def path_matches(path: str, filter_path: str, project_root: str = "", mcp: bool = True) -> bool:
    """The reference's filter_path test of one result path: both normalised, the project root stripped, a leading `/`
    and `./` trimmed from the path and `./` from the filter, then a prefix test.  MCP (src/mcp/mod.rs:400-425) also
    trims the filter's trailing `/`; the CLI (src/search/mod.rs:700-705, :728-738) does not."""
    root = _trim_end(normalize_path_str(project_root), "/")
    p = normalize_path_str(path)
    if p.startswith(root):
        p = p[len(root):]
    p = _trim_start(_trim_start(p, "/"), "./")
    f = _trim_start(normalize_path_str(filter_path), "./")
    if mcp:
        f = _trim_end(f, "/")
    return p.startswith(f)


def cap_per_group(cos, ids, groups, k: int, m: int):
    """The contract of the grouped search (cs_index_search_grouped) on the host: `cos` / `ids` are rows already in
    (cosine desc, id asc) order and `groups` their groups; walk them, keep a row whose group is NO_GROUP or has fewer
    than m rows kept, stop at k.  -> (cos, ids) of the kept rows, as lists."""
    kept_cos, kept_ids, have = [], [], {}
    for c, i, g in zip(cos, ids, groups):
        if len(kept_ids) >= k:
            break
        g = int(g)
        if g != NO_GROUP:
            if have.get(g, 0) >= m:
                continue
            have[g] = have.get(g, 0) + 1
        kept_cos.append(c)
        kept_ids.append(int(i))
    return kept_cos, kept_ids


def boost_order(cos, ids, classes, weights, k: int):
    """The contract of the boosted search (cs_index_search_boosted) on the host, in numpy float32: `cos` / `ids` are the
    live rows in (cosine desc, id asc) order — the full order, not a top-k: that is the point — and `classes` their classes
    (NO_CLASS: none).  s = 1 - (1 - c) * 0.5 (cos_to_score), b = s * w with one rounding, w = weights[class] for a class
    below len(weights) and 1 otherwise (weights None: every row weighs 1); the answer is the k rows with the largest
    key_pack(b, id): b descending, then id ascending.  -> (score, cos, ids) of those rows as arrays, best first."""
    import numpy as np

    from .sharded import key_pack
    from .vector_store import NO_CLASS, cos_to_score

    cos = np.asarray(cos, np.float32).ravel()
    ids = np.asarray(ids, np.uint32).ravel()
    cls = np.asarray(classes, np.int64).ravel()
    wt = np.zeros(0, np.float32) if weights is None else np.asarray(weights, np.float32).ravel()
    covered = (cls != NO_CLASS) & (cls >= 0) & (cls < wt.size)
    w = np.ones(cos.size, np.float32)
    w[covered] = wt[cls[covered]]
    b = (cos_to_score(cos) * w).astype(np.float32)
    order = np.argsort(key_pack(b, ids), kind="stable")[::-1][:max(int(k), 0)]
    return b[order], cos[order], ids[order]


def drop_excluded(cos, ids, groups, src_id: int, src_group: int, mode: str, min_cos, k: int):
    """The contract of the similar-chunk search (cs_index_search_similar) on the host: `cos` / `ids` are the live rows in
    (cosine desc, id asc) order for the source's stored row as the query, `groups` their groups.  mode "none" drops
    nothing, "self" the source chunk, "file" the source chunk and — when src_group is not NO_GROUP — every row of that
    group; then rows whose cosine is not strictly greater than min_cos go (None or -inf: no bound) and the first k stay.
    -> (cos, ids) of the kept rows, as lists."""
    if mode not in ("none", "self", "file"):
        raise ValueError(f'mode must be "none", "self" or "file", got {mode!r}')
    src_id, src_group = int(src_id), int(src_group)
    kept_cos, kept_ids = [], []
    for c, i, g in zip(cos, ids, groups):
        if len(kept_ids) >= k:
            break
        if mode != "none" and int(i) == src_id:
            continue
        if mode == "file" and src_group != NO_GROUP and int(g) == src_group:
            continue
        if min_cos is not None and not (c > min_cos):
            continue
        kept_cos.append(c)
        kept_ids.append(int(i))
    return kept_cos, kept_ids


def pairs_above(full_orders, group_of, mode: str, min_cos, max_pairs: int):
    """The contract of the similar-pairs search (cs_index_similar_pairs) on the host.  `full_orders`: {source id a: (cos,
    ids)}, per live chunk a the live chunks with the cosines the similar-chunk search reports for source a — the full order
    or any part of it that holds every hit that matters (hits b <= a are ignored: a pair is taken from its lower id);
    `group_of(ids)` -> their groups.  Take every pair a < b; mode "all" drops nothing, "other_group" the pairs whose two
    chunks carry the same group other than NO_GROUP; then pairs whose cosine is not strictly greater than min_cos go (None
    or -inf: no bound), and so do NaN / Inf cosines; order by (cosine desc, a asc, b asc).
    -> (cos, a, b, total): the first min(total, max_pairs) pairs as lists, and how many pairs remain in all."""
    if mode not in ("all", "other_group"):
        raise ValueError(f'mode must be "all" or "other_group", got {mode!r}')
    kept = []
    for a, (cos, ids) in full_orders.items():
        a = int(a)
        ids = [int(i) for i in ids]
        ga = int(group_of([a])[0])
        groups = group_of(ids) if mode == "other_group" else None
        for j, (c, b) in enumerate(zip(cos, ids)):
            if b <= a:
                continue
            if groups is not None and ga != NO_GROUP and int(groups[j]) == ga:
                continue
            if not (float("-inf") < c < float("inf")):
                continue
            if min_cos is not None and not (c > min_cos):
                continue
            kept.append((c, a, b))
    kept.sort(key=lambda t: (-float(t[0]), t[1], t[2]))
    top = kept[:max_pairs]
    return [t[0] for t in top], [t[1] for t in top], [t[2] for t in top], len(kept)


def pairs_between(cos, a, b, in_a, in_b):
    """The rule of the scoped similar-pairs search (cs_index_similar_pairs_scoped) on the host, as a filter over an
    unscoped answer: `cos` / `a` / `b` are the pairs of cs_index_similar_pairs (a < b, ordered by cosine desc, a asc, b asc,
    neither refused nor cut); `in_a` / `in_b` the ids of the two scopes (the same collection twice: the pairs inside one).
    A pair stays when one of its ids is in A and the other in B, either way round — once, however A and B overlap: the
    input holds every unordered pair once.  The order is kept.  -> (cos, a, b, total) with cos float32, a and b uint32."""
    import numpy as np

    cos = np.asarray(cos, np.float32).ravel()
    a = np.asarray(a, np.uint32).ravel()
    b = np.asarray(b, np.uint32).ravel()
    sa = np.unique(np.asarray(list(in_a) if not isinstance(in_a, np.ndarray) else in_a, np.uint32))
    sb = np.unique(np.asarray(list(in_b) if not isinstance(in_b, np.ndarray) else in_b, np.uint32))
    keep = (np.isin(a, sa) & np.isin(b, sb)) | (np.isin(a, sb) & np.isin(b, sa))
    return cos[keep], a[keep], b[keep], int(keep.sum())


def clusters_of_pairs(live_ids, a, b):
    """The contract of the similar-clusters search (cs_index_similar_clusters) on the host, as a reduction of a pair list:
    `live_ids` are the vertices, (a[i], b[i]) the edges — the pairs of cs_index_similar_pairs with the same bound and mode,
    neither refused nor cut.  Union by smallest id: the label of an id is the smallest id of its connected component, an id
    without an edge is its own label.  An edge that names an id not in live_ids is a ValueError (the pairs call never
    returns one); a repeated edge, or (a, b) given as (b, a), changes nothing.
    -> (labels, clusters, members): {id: label} over live_ids, the components of two or more ids, the ids in them."""
    parent = {int(i): int(i) for i in live_ids}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for x, y in zip(a, b):
        x, y = int(x), int(y)
        if x not in parent or y not in parent:
            raise ValueError(f"pair ({x}, {y}) names an id that is not live")
        rx, ry = find(x), find(y)
        if rx != ry:
            parent[max(rx, ry)] = min(rx, ry)  # the smaller root stays a root: a root is its component's smallest id
    labels = {i: find(i) for i in parent}
    sizes = {}
    for root in labels.values():
        sizes[root] = sizes.get(root, 0) + 1
    big = [n for n in sizes.values() if n >= 2]
    return labels, len(big), sum(big)


def merge_variants_capped(lists, group_of, k: int, m: int):
    """The contract of the grouped variants search (cs_index_search_variants_grouped[_scoped]) on the host.  `lists`: per
    query variant a (cos, ids) pair over the rows in play — the variant's full order, or any list that holds every row
    that matters; `group_of(ids)` -> their groups.  A chunk keeps its best cosine over the variants (the best packed key:
    cosine desc, then id asc, so of one id simply the largest cosine), the chunks are ordered by (that cosine desc, id asc)
    and capped by cap_per_group.  -> (cos, ids) of the kept rows, as lists."""
    best = {}
    for cos, ids in lists:
        for c, i in zip(cos, ids):
            i = int(i)
            if i not in best or c > best[i]:
                best[i] = c
    order = sorted(best, key=lambda i: (-float(best[i]), i))
    return cap_per_group([best[i] for i in order], order, group_of(order) if order else [], k, m)


def merge_variants_boosted(lists, class_of, weights, k: int, group_of=None, m: Optional[int] = None):
    """The contract of the boosted variants searches (cs_index_search_variants_boosted and its _scoped / _grouped forms) on
    the host, in numpy float32.  `lists`: per query variant a (cos, ids) pair over the rows in play — the variant's FULL
    order (a boosted row just outside a top-k is the point), every row once per variant; `class_of(ids)` -> their classes,
    `group_of(ids)` -> their groups.  A chunk keeps c = its best cosine over the variants; b = f32(cos_to_score(c) * w) by
    boost_order's arithmetic, which is also the best of its per-variant boosted scores; the chunks are ordered by
    key_pack(b, id) — b descending, then id ascending — and, when group_of and m are given, capped by cap_per_group's walk
    over that order.  -> (score, cos, ids) of the first k kept rows as arrays, best first."""
    import numpy as np

    cos = np.concatenate([np.asarray(c, np.float32).ravel() for c, _ in lists]) if len(lists) else np.zeros(0, np.float32)
    ids = np.concatenate([np.asarray(i, np.uint32).ravel() for _, i in lists]) if len(lists) else np.zeros(0, np.uint32)
    order = np.lexsort((-cos, ids))  # by id, a chunk's best cosine first
    cos, ids = cos[order], ids[order]
    first = np.ones(ids.size, bool)
    first[1:] = ids[1:] != ids[:-1]
    cos, ids = cos[first], ids[first]
    capped = group_of is not None and m is not None
    b, c, i = boost_order(cos, ids, class_of(ids) if ids.size else [], weights, ids.size if capped else k)
    if capped and i.size:
        pos, _ = cap_per_group(range(i.size), i, group_of(i), k, m)
        pos = np.asarray(pos, np.int64)
        b, c, i = b[pos], c[pos], i[pos]
    return b[:max(int(k), 0)], c[:max(int(k), 0)], i[:max(int(k), 0)]


def high_confidence(cos, top_n: int = 5, max_distance: float = 0.15) -> bool:
    """The early-termination predicate of the variants searches on a returned list's cosines (src/search/mod.rs:595-611):
    the list is not empty and its first top_n entries all have distance (1 - cos) / 2 < max_distance, in float32."""
    c = np.asarray(cos, np.float32)[:top_n]
    return bool(len(c)) and bool(((np.float32(1.0) - c) * np.float32(0.5) < np.float32(max_distance)).all())


def group_results_by_file(results: Sequence[SearchResult], per_file: Optional[int],
                          max_results: Optional[int] = None) -> List[SearchResult]:
    """The reference's display order under `--per-file` (src/search/mod.rs:1007-1038): the results grouped by path, the
    files ordered by their best score (descending; as there the best score counts as at least 0), the hits of a file by
    score, at most per_file of them.  per_file None or 0, or not below max_results when that is given: the results as
    they are (mod.rs:1009, :1039-1044).  Equal scores keep the order they came in (the reference's HashMap leaves it open).
    After VectorStore.search(per_file=...) the truncation drops nothing: the cap was applied before the top-k."""
    results = list(results)
    if not per_file or per_file <= 0 or (max_results is not None and per_file >= max_results):
        return results
    by_file: Dict[str, List[SearchResult]] = {}
    for r in results:
        by_file.setdefault(r.path, []).append(r)
    files = sorted(by_file.values(), key=lambda rs: -max([0.0] + [r.score for r in rs]))
    out: List[SearchResult] = []
    for rs in files:
        out.extend(sorted(rs, key=lambda r: -r.score)[:per_file])
    return out


class ScopeCache:
    """filter_path -> Scope of one store, for a server that answers the same `filter_path` over and over between two
    index builds: the directory's chunk ids are looked up and prepared on first use (VectorStore.chunk_ids_under ->
    VectorStore.scope) and searched from the device afterwards.  A scope's row list follows builds by itself; its ID
    list does not, so invalidate() after chunks were inserted or deleted — the scopes are dropped and remade lazily."""

    def __init__(self, store, project_root: str = "", mcp: bool = True):
        self.store, self.project_root, self.mcp = store, project_root, mcp
        self._scopes: Dict[str, Scope] = {}

    def get(self, filter_path: str) -> Scope:
        sc = self._scopes.get(filter_path)
        if sc is None:
            sc = self.store.scope(self.store.chunk_ids_under(filter_path, self.project_root, self.mcp))
            self._scopes[filter_path] = sc
        return sc

    def invalidate(self) -> None:
        for sc in self._scopes.values():
            sc.close()
        self._scopes.clear()

    close = invalidate

    def __len__(self) -> int:
        return len(self._scopes)


def vector_search_step(store, query_embeddings, limit: int, filter_path: Optional[str] = None,
                       scopes: Optional[ScopeCache] = None, project_root: str = "", mcp: bool = True):
    """search::search's vector leg (VectorStore.search_variants) narrowed to `filter_path` BEFORE the top-k instead of
    after it (the reference post-filters the top limit * 3: src/mcp/mod.rs:251-252,400-425): through the caller's
    ScopeCache where it holds one, else through a one-off masked search over the directory's chunk ids.
    -> (results, high_confidence)."""
    if filter_path is None:
        return store.search_variants(query_embeddings, limit)
    if scopes is not None:
        return store.search_variants(query_embeddings, limit, scope=scopes.get(filter_path))
    return store.search_variants(query_embeddings, limit, chunk_ids=store.chunk_ids_under(filter_path, project_root, mcp))


def should_use_vector_only(results: Sequence[SearchResult], vector_only: bool) -> bool:
    """mod.rs:601-611: skip FTS when the top-5 all have distance < 0.15."""
    if vector_only:
        return False
    top = list(results[:EARLY_TERMINATION_TOP_N])
    return bool(top) and all(r.distance < HIGH_CONFIDENCE_THRESHOLD for r in top)


# ---- result fusion (/root/reference/src/rerank/mod.rs:14-241) -----------------------------------
import dataclasses
from typing import Dict, Optional, Tuple

import numpy as np

DEFAULT_RRF_K = 20.0      # rerank/mod.rs:15
EXACT_MATCH_RRF_K = 5.0   # rerank/mod.rs:18


@dataclasses.dataclass
class FusedResult:
    """rerank/mod.rs:21-36."""
    chunk_id: int
    rrf_score: float
    vector_score: Optional[float] = None
    fts_score: Optional[float] = None
    vector_rank: Optional[int] = None
    fts_rank: Optional[int] = None


def _rrf_term(k: float, rank0: int) -> np.float32:
    # `1.0 / (k + rank as f32 + 1.0)` in f32, rerank/mod.rs:59
    return np.float32(1.0) / (np.float32(k) + np.float32(rank0) + np.float32(1.0))


def _sorted_desc(results: List[FusedResult]) -> List[FusedResult]:
    # rerank/mod.rs:101-105: sort by rrf_score descending (stable; the reference's input order is a
    # HashMap's, i.e. unspecified between equal scores — here first-seen order)
    return sorted(results, key=lambda r: -r.rrf_score)


def rrf_fusion(vector_results: Sequence[SearchResult], fts_results: Sequence[Tuple[int, float]],
               k: float = DEFAULT_RRF_K) -> List[FusedResult]:
    """rerank/mod.rs:48-108.  fts_results: (chunk_id, bm25 score) in rank order (FtsResult)."""
    acc: Dict[int, FusedResult] = {}
    for rank, r in enumerate(vector_results):
        e = acc.setdefault(r.id, FusedResult(r.id, np.float32(0.0)))
        e.rrf_score = np.float32(e.rrf_score + _rrf_term(k, rank))
        e.vector_score, e.vector_rank = r.score, rank + 1
    for rank, (cid, score) in enumerate(fts_results):
        e = acc.setdefault(cid, FusedResult(cid, np.float32(0.0)))
        e.rrf_score = np.float32(e.rrf_score + _rrf_term(k, rank))
        e.fts_score, e.fts_rank = score, rank + 1
    out = _sorted_desc(list(acc.values()))
    for e in out:
        e.rrf_score = float(e.rrf_score)
    return out


def vector_only(vector_results: Sequence[SearchResult]) -> List[FusedResult]:
    """rerank/mod.rs:111-124: pass-through, rrf_score = the vector score."""
    return [FusedResult(r.id, r.score, r.score, None, rank + 1, None) for rank, r in enumerate(vector_results)]


def rrf_fusion_with_exact(vector_results: Sequence[SearchResult], fts_results: Sequence[Tuple[int, float]],
                          exact_results: Sequence[Tuple[int, float]], vector_k: float = DEFAULT_RRF_K,
                          fts_k: float = DEFAULT_RRF_K, exact_k: float = EXACT_MATCH_RRF_K) -> List[FusedResult]:
    """rerank/mod.rs:139-241: three-way fusion; exact identifier matches get the smaller k.  The
    fts_score of a result is the mean of its FTS and exact scores when both exist (:216-221) and its
    fts_rank falls back to the exact rank (:229)."""
    acc: Dict[int, list] = {}  # id -> [rrf, vscore, fscore, escore, vrank, frank, erank]

    def entry(cid):
        return acc.setdefault(cid, [np.float32(0.0), None, None, None, None, None, None])

    for rank, r in enumerate(vector_results):
        e = entry(r.id)
        e[0] = np.float32(e[0] + _rrf_term(vector_k, rank)); e[1] = r.score; e[4] = rank + 1
    for rank, (cid, score) in enumerate(fts_results):
        e = entry(cid)
        e[0] = np.float32(e[0] + _rrf_term(fts_k, rank)); e[2] = score; e[5] = rank + 1
    for rank, (cid, score) in enumerate(exact_results):
        e = entry(cid)
        e[0] = np.float32(e[0] + _rrf_term(exact_k, rank)); e[3] = score; e[6] = rank + 1
    out = []
    for cid, (rrf, vs, fs, es, vr, fr, er) in acc.items():
        if fs is not None and es is not None:
            comb = float((np.float32(fs) + np.float32(es)) / np.float32(2.0))
        else:
            comb = fs if fs is not None else es
        out.append(FusedResult(cid, float(rrf), vs, comb, vr, fr if fr is not None else er))
    return _sorted_desc(out)


# ---- the neural second pass (/root/reference/src/search/mod.rs:712-722, :829-885) ----------------

def rerank_take_count(n_fused: int, max_results: int, rerank: bool, rerank_top: Optional[int] = None,
                      filter_by_path: bool = False) -> int:
    """mod.rs:712-722: how many fused results go on — `rerank_top` (default max_results) of them when the reranker is on,
    else max_results (three times as many under a path filter)."""
    if rerank:
        return min(rerank_top if rerank_top is not None else max_results, n_fused)
    return max_results * (3 if filter_by_path else 1)


def rerank_step(reranker, query: str, results: Sequence[SearchResult], max_results: int,
                filter_path: Optional[str] = None, project_root: str = "") -> List[SearchResult]:
    """mod.rs:829-885: rerank_and_blend over the results' contents with their (fusion) scores, reorder with the blended
    score as the new score, the post-reranking path filter, truncate to max_results.  `reranker`: a rerank.NeuralReranker
    (None, or no results: the results go through unreranked, as when the reference's reranker is off)."""
    results = list(results)
    if reranker is not None and results:
        reranked = reranker.rerank_and_blend(query, [r.content for r in results], [r.score for r in results])
        results = [dataclasses.replace(results[idx], score=score) for idx, score in reranked]
    if filter_path is not None:
        results = [r for r in results if path_matches(r.path, filter_path, project_root, mcp=False)]
    return results[:max_results]
