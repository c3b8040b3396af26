"""Boosted search across query variants, in a scope, under the per-file cap (cs_index_search_variants_boosted and its
_scoped / _grouped / _grouped_scoped forms; codesearch_amd/csrc/scan_boosted_grouped.hip): a chunk keeps its best cosine c
over the variants, b = f32(score(c) * weight of its class), the rows are ordered by (b desc, id asc) and, in the grouped
forms, walked under the cap.

Ground truth comes only from code that exists without the feature: each variant's full (cosine desc, id asc) order of a
store of at most 1,024 live rows — one streaming search_raw(q, n), with its cosine bits — passed through
search.merge_variants_boosted; for larger stores the boosted search of each variant.  Ids, the bytes of out_score and of
out_cos, the count and the flag must all match exactly."""
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, boost_order, cap_per_group, high_confidence, merge_variants_boosted
from codesearch_amd.sharded import key_pack
from codesearch_amd.synth import synth_rows
from codesearch_amd.vector_store import CHUNK_KINDS, NO_CLASS, cos_to_score

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF
MAX_VARIANTS = 16  # CS_MAX_VARIANTS
f32 = np.float32
SHAPES = [(1, 1), (10, 1), (10, 3), (10, 9), (200, 9), (500, 9), (1000, 16)]  # (k, nq); the last two: two merge levels


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows, id_base=0):
    st = VS(None, rows.shape[1], id_base=id_base)
    st.insert_embeddings(rows)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    return st


def _scope(st, ids):
    sc = st.scope(ids)
    sc.set_route("gather")
    return sc


def _full_order(st, q):
    """(cos, ids) of every live row of a store of at most 1,024 live rows, (cosine desc, id asc): one streaming search."""
    n = len(st)
    assert 0 < n <= 1024
    c, i, cnt = st.search_raw(q, n)
    assert cnt[0] == n
    return c[0].copy(), i[0].copy()


def _lookup(table: dict, none):
    return lambda ids: [table.get(int(i), none) for i in ids]


def _kind_weights(kind, w):
    t = np.ones(len(CHUNK_KINDS), f32)
    t[kind] = w
    return t


def _same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


def _matches(got, want, what):
    """got = search_variants_raw(class_weights=)'s five; want = (score, cos, ids) of the kept rows, best first."""
    score, cos, ids, count, flag = got
    es, ec, ei = (np.asarray(x) for x in want)
    n = len(ei)
    assert count == n, (what, count, n)
    assert ids[:n].tolist() == ei.tolist(), what
    assert score[:n].tobytes() == es.astype(f32).tobytes(), what
    assert cos[:n].tobytes() == ec.astype(f32).tobytes(), what
    assert (ids[n:] == NO_ID).all() and (cos[n:] == 0).all() and (score[n:] == 0).all(), what
    assert flag == high_confidence(ec), what


def _inside(truth, ids):
    """The variants' full orders restricted to the ids of a scope (None: every id)."""
    return truth if ids is None else [(c[np.isin(i, ids)], i[np.isin(i, ids)]) for c, i in truth]


def _check(st, lists, class_of, weights, group_of, qs, k, m=None, scope=None):
    """st.search_variants_raw(qs, k, class_weights=weights[, per_file=m][, scope=]) against the variants' full orders
    `lists` (of the scope's rows, for a scope: _inside) merged, boosted and capped on the host."""
    want = merge_variants_boosted(lists[:len(qs)], class_of, weights, k, group_of if m is not None else None, m)
    got = st.search_variants_raw(qs, k, scope=scope, per_file=m, class_weights=weights)
    _matches(got, want, (k, len(qs), m, scope is not None))
    return got


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_equals_the_variants_full_orders_boosted_and_capped(VS, dim):
    n, seed = 1000, 9500 + dim
    rows = synth_rows(seed, 0, n, dim)
    qs = np.concatenate([synth_rows(seed + 1, 0, 14, dim), rows[[5, n - 3]]])
    st = _store(VS, rows)
    truth = [_full_order(st, q) for q in qs]
    every, third = np.arange(n), np.arange(0, n, 3)
    forms = [(None, truth), (_scope(st, third), _inside(truth, third)), (_scope(st, every), _inside(truth, every))]
    gathered = [sc.route_info()[1] if sc else 0 for sc, _ in forms]
    rng = np.random.default_rng(seed)
    by_kind = {r: r % 18 for r in range(n)}
    classings = [  # test_boosted_equals_boosted_full_order's
        ("none", {}, _kind_weights(3, 1.15)),
        ("kind at 1.15", by_kind, _kind_weights(3, 1.15)),
        ("63 classes, random weights", {r: r // 16 for r in range(n)}, rng.uniform(0.5, 1.5, 63).astype(f32)),
        ("one class weighs 0", by_kind, _kind_weights(5, 0.0)),
        ("a table shorter than the classes", by_kind, rng.uniform(0.5, 1.5, 7).astype(f32)),
    ]
    groupings = [("none", {}), ("files of 8", {r: r // 8 for r in range(n)}), ("id % 5", {r: r % 5 for r in range(n)})]
    calls = 0
    for cname, classes, weights in classings:
        if classes:
            st.set_classes(list(classes), list(classes.values()))
        class_of = _lookup(classes, NO_CLASS)
        for gname, groups in groupings:
            st.set_groups(every, [groups.get(r, NO_GROUP) for r in range(n)])
            group_of = _lookup(groups, NO_GROUP)
            for k, nq in SHAPES:
                for m in (None, 1, 3, k):
                    calls += 1
                    for sc, lists in forms:
                        _check(st, lists, class_of, weights, group_of, qs[:nq], k, m, sc)
    for (sc, _), before in zip(forms, gathered):  # the scoped forms always take the gathered scan
        if sc:
            assert sc.route_info()[0] == 0 and sc.route_info()[1] - before == calls
            sc.close()
    st.close()


@pytest.mark.parametrize("n,dim", [(1000, 384), (1000, 100), (5000, 768)])
def test_the_identities_of_the_contract(VS, n, dim):
    rows = synth_rows(9600 + dim, 0, n, dim)
    qs = synth_rows(9601 + dim, 0, 9, dim)
    st = _store(VS, rows)
    st.set_classes(np.arange(n), np.arange(n) % 18)
    w = _kind_weights(3, 1.15)
    everything, half = _scope(st, np.arange(n)), _scope(st, np.arange(0, n, 2))
    for k in (1, 10, 200, 1000):
        # one variant, uncapped: the boosted search of that query
        for sc in (None, half):
            s, c, i, cnt = st.search_raw(qs[0], k, class_weights=w, scope=sc)
            one = st.search_variants_raw(qs[0], k, class_weights=w, scope=sc)
            assert _same(one[:3], (s[0], c[0], i[0])) and one[3] == cnt[0]
        for nq in (1, 3, 9):
            plain = st.search_variants_raw(qs[:nq], k, class_weights=w)
            half_plain = st.search_variants_raw(qs[:nq], k, class_weights=w, scope=half)
            assert plain[3] == min(k, n) and half_plain[3] == min(k, n // 2)
            # no group assigned: a grouped form is its uncapped sibling
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=1), plain)
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=1, scope=half), half_plain)
            st.set_groups(np.arange(n), np.arange(n) // 8)
            # a cap that cannot bind
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=k), plain)
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=k + 5, scope=half), half_plain)
            # a scope that holds every id
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, scope=everything), plain)
            capped = st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=2)
            assert _same(st.search_variants_raw(qs[:nq], k, class_weights=w, per_file=2, scope=everything), capped)
            st.set_groups(np.arange(n), np.full(n, NO_GROUP))
    # no table: b is the score, and the ids are those of the plain variants search up to ties in the score
    s, c, i, cnt, flag = st.search_variants_raw(qs[:3], 10, class_weights=np.zeros(0, f32))
    assert s.tobytes() == cos_to_score(c).astype(f32).tobytes()
    pc, pi, pn, pf = st.search_variants_raw(qs[:3], 10)
    assert sorted(i.tolist()) == sorted(pi.tolist()) and flag == pf
    everything.close()
    half.close()
    st.close()


CLOSE = np.array([0.99, 1.0, 1.01], f32)  # within the spread of the best scores, so the answer mixes the classes


def _merged_boosted_lists(st, qs, k, values):
    """Per variant the boosted top k (cs_index_search_boosted), merged: {id: (best b, best cos)} and the largest last b."""
    score, cos, ids, cnt = st.search_raw(qs, k, class_weights=values)
    assert (cnt == k).all()
    best = {}
    for q in range(len(qs)):
        for b, c, i in zip(score[q].tolist(), cos[q].tolist(), ids[q].tolist()):
            pb, pc = best.get(i, (b, c))
            best[i] = (max(pb, b), max(pc, c))
    return best, float(score[:, -1].max())


def _by_key(best):
    ids = np.array(list(best), np.uint32)
    b = np.array([best[int(i)][0] for i in ids], f32)
    c = np.array([best[int(i)][1] for i in ids], f32)
    order = np.argsort(key_pack(b, ids))[::-1]
    return b[order], c[order], ids[order]


@pytest.mark.parametrize("n,k", [(20_000, 10), (120_000, 200)])
def test_more_rows_than_a_list_holds_uncapped(VS, n, k):
    """Truth: each variant's boosted search (a row of the merged top k is in the boosted top k of every variant in which
    it reaches its best b), the best b per id, the first k by key.  120,000 rows at k = 200 run behind the prime pass."""
    dim = 384
    qs = synth_rows(9701, 0, 3, dim)
    st = VS(None, dim)
    st.insert_synthetic(n, 9700, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    cls = (np.arange(n) * 7 % 3).astype(np.uint16)
    st.set_classes(np.arange(n), cls)
    best, _ = _merged_boosted_lists(st, qs, k, CLOSE)
    b, c, i = _by_key(best)
    got = st.search_variants_raw(qs, k, class_weights=CLOSE)
    _matches(got, (b[:k], c[:k], i[:k]), (n, k))
    assert len(set(cls[got[2]].tolist())) > 1
    everything = _scope(st, np.arange(n))
    assert _same(st.search_variants_raw(qs, k, class_weights=CLOSE, scope=everything), got)
    assert _same(st.search_variants_raw(qs, k, class_weights=CLOSE, per_file=1), got)  # no group assigned
    everything.close()
    st.close()


@pytest.mark.parametrize("k", [10, 200])
def test_more_rows_than_a_list_holds_capped(VS, k):
    """20,000 rows, files of 8, at most one row per file.  Per variant the boosted top 1,024; T = the largest of the three
    lists' last b.  Every row whose merged b exceeds T is in the merged list with its true key, so the capped walk over the
    merged list is the contract's as long as it keeps k rows before it reaches b <= T — asserted on the truth alone."""
    n, dim, m = 20_000, 384, 1
    qs = synth_rows(9711, 0, 3, dim)
    st = VS(None, dim)
    st.insert_synthetic(n, 9710, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    cls = (np.arange(n) * 7 % 3).astype(np.uint16)
    st.set_classes(np.arange(n), cls)
    groups = (np.arange(n) // 8).astype(np.uint32)
    st.set_groups(np.arange(n), groups)
    best, T = _merged_boosted_lists(st, qs, 1024, CLOSE)
    b, c, i = _by_key(best)
    pos, kept = cap_per_group(range(i.size), i, groups[i], k, m)
    assert len(kept) == k and b[pos[-1]] > T  # the walk ends inside the part of the order the lists pin down
    pos = np.asarray(pos)
    got = st.search_variants_raw(qs, k, class_weights=CLOSE, per_file=m)
    _matches(got, (b[pos], c[pos], i[pos]), k)
    assert len(set(groups[got[2]].tolist())) == k
    everything = _scope(st, np.arange(n))
    assert _same(st.search_variants_raw(qs, k, class_weights=CLOSE, per_file=m, scope=everything), got)
    everything.close()
    st.close()


def test_follows_the_store_life_cycle(VS):
    n, dim, base = 1000, 384, 1000
    rows = synth_rows(9900, 0, n, dim)
    qs = synth_rows(9901, 0, 9, dim)
    st = _store(VS, rows, id_base=base)
    classes = {base + r: r % 18 for r in range(n)}
    groups = {base + r: r // 8 for r in range(n)}
    st.set_classes(list(classes), list(classes.values()))
    st.set_groups(list(groups), list(groups.values()))
    weights = np.random.default_rng(3).uniform(0.5, 1.5, 18).astype(f32)
    class_of, group_of = _lookup(classes, NO_CLASS), _lookup(groups, NO_GROUP)
    issued = np.arange(base, base + n + 6)
    third = issued[::3]
    scopes = [(None, None), (_scope(st, third), third), (_scope(st, issued), issued)]

    def check_all():
        truth = [_full_order(st, q) for q in qs]
        out = None
        for k, nq in [(10, 1), (10, 9), (200, 9), (len(st), 3)]:  # every live row: each winner's row is found again
            for m in (None, 1, 3):
                for sc, inside in scopes:
                    got = _check(st, _inside(truth, inside), class_of, weights, group_of, qs[:nq], k, m, sc)
                    out = out or got
        return out

    check_all()
    # 5 % deleted: the build leaves tombstones, and the unscoped capped scan reads the dead-row bitmap
    dead = [base + r for r in range(0, n, 20)]
    assert st.delete_chunks(dead) == len(dead)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.stored_rows() == n and len(st) == n - len(dead)
    check_all()
    # 30 % more: the build reclaims them, row != id - id_base from here on (the bisection of the cosine pass)
    more = [base + r for r in range(n) if r % 20 and r % 10 in (3, 6, 9)]
    assert st.delete_chunks(more) == len(more) == 300
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.stored_rows() == len(st) == n - len(dead) - 300
    check_all()
    # rows appended after the assignments carry neither class nor group: they weigh 1 and are never capped
    new = st.insert_embeddings(np.stack([0.95 * qs[0] + 0.05 * rows[j] for j in range(6)])).tolist()
    assert new == issued[-6:].tolist()
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    score, cos, ids, count, flag = check_all()  # (k, nq, m) = (10, 1, None), unscoped
    assert sorted(ids[:6].tolist()) == new and score[:6].tobytes() == cos_to_score(cos[:6]).astype(f32).tobytes()
    assert st.search_variants_raw(qs[:1], 10, class_weights=weights, per_file=1)[2][:6].tolist() == ids[:6].tolist()
    for sc, _ in scopes:
        if sc:
            sc.close()
    st.close()


def _chunks(rows, kinds, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, kinds[i], paths[i]), rows[i]) for i in range(len(rows))]


def test_a_hog_file_of_the_boosted_kind(VS):
    """What the combination is for.  One file holds 60 near-duplicates of the query and they carry the boosted kind: the
    call at one hit per file returns 10 files; boosting and capping the merged variants list on the host — what a caller
    had to do — sees the hog file only and returns fewer."""
    n, dim, k = 500, 384, 10
    rows = synth_rows(9800, 0, n, dim)
    q = synth_rows(9801, 0, 1, dim)[0]
    qs = np.stack([q, 0.98 * q + 0.02 * synth_rows(9802, 0, 1, dim)[0]])
    hog = np.arange(200, 260)
    rows[hog] = 0.9 * q + 0.1 * rows[hog]
    kinds = ["Struct" if 200 <= r < 260 else "Function" for r in range(n)]
    paths = ["src/hog.rs" if 200 <= r < 260 else f"src/f{r // 8}.rs" for r in range(n)]
    st = VS(None, dim)
    ids = st.insert_chunks_with_ids(_chunks(rows, kinds, paths))
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert ids == list(range(n)) and st.classes_info()[0] == n and st.groups_info()[0] == n
    res, flag = st.search_variants(qs, k, per_file=1, boost_kind="Struct", boost=0.15)
    assert len(res) == k and len({r.path for r in res}) == k and sum(r.path == "src/hog.rs" for r in res) == 1
    assert res[0].path == "src/hog.rs" and not flag
    w = _kind_weights(CHUNK_KINDS.index("Struct"), f32(1.0) + f32(0.15))
    score, cos, got, count, _ = st.search_variants_raw(qs, k, per_file=1, class_weights=w)
    assert count == k and got.tolist() == [r.id for r in res] and [f32(r.score) for r in res] == score.tolist()
    assert f32(res[0].score) == f32(cos_to_score(cos[0]) * w[3]) and f32(res[0].distance) == f32((f32(1) - cos[0]) * f32(0.5))
    # the same against the full orders
    truth = [_full_order(st, v) for v in qs]
    file_of = {r: (0 if 200 <= r < 260 else 1 + r // 8) for r in range(n)}
    es, ec, ei = merge_variants_boosted(truth, lambda i: [CHUNK_KINDS.index(kinds[int(x)]) for x in i], w, k,
                                        lambda i: [file_of[int(x)] for x in i], 1)
    assert ei.tolist() == got.tolist() and es.tobytes() == score.tobytes() and ec.tobytes() == cos.tobytes()
    # rank, merge, then boost and cap on the host
    pc, pi, pn, _ = st.search_variants_raw(qs, k)
    assert set(pi.tolist()) <= set(hog.tolist())
    bs, bc, bi = boost_order(pc, pi, [CHUNK_KINDS.index(kinds[int(x)]) for x in pi], w, k)
    assert len(cap_per_group(bc, bi, [file_of[int(x)] for x in bi], k, 1)[1]) == 1 < k
    # in a scope without the hog's best rows the answer follows
    sc = _scope(st, np.r_[0:205, 255:n])
    inside = st.search_variants_raw(qs, k, per_file=1, class_weights=w, scope=sc)
    assert inside[3] == k and sum(200 <= i < 260 for i in inside[2].tolist()) == 1
    assert not any(205 <= i < 255 for i in inside[2].tolist())
    sc.close()
    st.close()


def test_the_flag_reads_the_cosines_of_the_list_returned(VS):
    """Five rows identical to the query: distance 0, the flag is set — from c, though the keys carry b (here 0.5 * score,
    which as a cosine would be far).  Under a cap of one per file it stays set only if the five are in different files."""
    n, dim = 300, 384
    rows = synth_rows(9810, 0, n, dim)
    q = synth_rows(9811, 0, 1, dim)[0]
    twins = [7, 70, 133, 200, 299]
    rows[twins] = q
    st = _store(VS, rows)
    st.set_classes(np.arange(n), np.zeros(n, np.uint16))
    half = np.array([0.5], f32)
    qs = np.stack([q, synth_rows(9812, 0, 1, dim)[0]])
    for kw in ({}, {"per_file": 1}):
        score, cos, ids, count, flag = st.search_variants_raw(qs, 10, class_weights=half, **kw)
        assert ids[:5].tolist() == twins and flag and count == 10 and (score[:5] < 0.51).all() and (cos[:5] > 0.999).all()
        assert not st.search_variants_raw(qs[1:], 10, class_weights=half, **kw)[4]  # nothing near the second variant
        assert st.search_variants_raw(qs, 3, class_weights=half, **kw)[4]           # fewer than five returned: all of them
    st.set_groups(twins, [9] * 5)  # one file: the cap keeps one twin, and the next rows are far from the query
    score, cos, ids, count, flag = st.search_variants_raw(qs, 10, class_weights=half, per_file=1)
    assert ids[0] == twins[0] and not set(ids[1:].tolist()) & set(twins) and not flag
    assert st.search_variants_raw(qs, 10, class_weights=half)[4]
    assert st.search_variants_raw(qs, 10, class_weights=half, per_file=5)[4]
    st.close()


def test_arguments(VS):
    n, dim, k = 300, 384, 5
    rows = synth_rows(9950, 0, n, dim)
    q = synth_rows(9951, 0, 2, dim)
    ones = np.ones(4, f32)
    st, other = VS(None, dim), VS(None, dim)
    st.insert_embeddings(rows)
    other.insert_embeddings(rows)
    sc, foreign = st.scope(np.arange(0, n, 2)), other.scope(np.arange(n))
    forms = [{}, {"scope": sc}, {"per_file": 1}, {"per_file": 1, "scope": sc}]
    for kw in forms:
        with pytest.raises(_lib.CsError, match="Index not built"):
            st.search_variants_raw(q, k, class_weights=ones, **kw)
    st.build_index()
    other.build_index()
    bad_w = ones.copy()
    bad_w[2] = np.nan
    many = np.repeat(q[:1], MAX_VARIANTS + 1, axis=0)
    for kw in forms:
        capped, scoped = "per_file" in kw, "scope" in kw
        # the search's own checks first, whatever else is wrong with the call
        wrong = dict(kw, per_file=0) if capped else kw
        wrong = dict(wrong, scope=foreign) if scoped else wrong
        with pytest.raises(_lib.CsError, match="Query embedding dimension mismatch: expected 384, got 100") as e:
            st.search_variants_raw(np.zeros((1, 100), f32), k, class_weights=bad_w, **wrong)
        assert e.value.code == _lib.CS_ERR_DIM_MISMATCH
        with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 1025"):
            st.search_variants_raw(q, 1025, class_weights=bad_w, **wrong)
        with pytest.raises(_lib.CsError, match=f"at most {MAX_VARIANTS} query variants per call, got {MAX_VARIANTS + 1}"):
            st.search_variants_raw(many, k, class_weights=bad_w, **wrong)
        if capped:  # then the cap's, before the table's and the scope's
            with pytest.raises(_lib.CsError, match="per_group must be at least 1") as e:
                st.search_variants_raw(q, k, class_weights=bad_w, **wrong)
            assert e.value.code == _lib.CS_ERR_BAD_ARG
            wrong = dict(wrong, per_file=1)
        with pytest.raises(_lib.CsError, match=r"weights\[2\]"):  # then the table's, before the scope's
            st.search_variants_raw(q, k, class_weights=bad_w, **wrong)
        with pytest.raises(_lib.CsError, match="n_classes must be at most 4096, got 4097"):
            st.search_variants_raw(q, k, class_weights=np.ones(4097, f32), **wrong)
        if scoped:
            with pytest.raises(_lib.CsError, match="the scope was made for another store") as e:
                st.search_variants_raw(q, k, class_weights=ones, **wrong)
            assert e.value.code == _lib.CS_ERR_BAD_ARG
        assert st.search_variants_raw(q, k, class_weights=ones, **kw)[3] == k
    # a null scope, and each output optional but one given
    lib, h = st._lib, st.handle
    qp, wp = q.ctypes.data_as(_lib.f32p), ones.ctypes.data_as(_lib.f32p)
    assert lib.cs_index_search_variants_boosted_scoped(h, None, qp, 2, dim, k, wp, 4, None, None, None, None, None) == _lib.CS_ERR_BAD_ARG
    assert "no output buffer" in _lib.last_error()
    ids = np.zeros(k, np.uint32)
    assert lib.cs_index_search_variants_boosted_scoped(h, None, qp, 2, dim, k, wp, 4, None, None, ids.ctypes.data_as(_lib.u32p),
                                                       None, None) == _lib.CS_ERR_BAD_ARG
    assert "null scope handle" in _lib.last_error()
    assert lib.cs_index_search_variants_boosted_grouped_scoped(h, None, qp, 2, dim, k, 1, wp, 4, None, None,
                                                               ids.ctypes.data_as(_lib.u32p), None, None) == _lib.CS_ERR_BAD_ARG
    assert "null scope handle" in _lib.last_error()
    want = st.search_variants_raw(q, k, class_weights=ones, per_file=1)
    _lib.check(lib.cs_index_search_variants_boosted_grouped(h, qp, 2, dim, k, 1, None, 0, None, None, ids.ctypes.data_as(_lib.u32p),
                                                            None, None))
    assert ids.tobytes() == want[2].tobytes()
    import ctypes

    flag = ctypes.c_int32(7)
    _lib.check(lib.cs_index_search_variants_boosted(h, qp, 2, dim, k, None, 0, None, None, None, None, ctypes.byref(flag)))
    assert flag.value == int(want[4])
    with pytest.raises(ValueError, match="exclusive with chunk_ids"):
        st.search_variants_raw(q, k, class_weights=ones, chunk_ids=[1, 2])
    with pytest.raises(ValueError, match="CHUNK_KINDS"):
        st.search_variants(q, k, boost_kind="Structure")
    # a scope with no live row, and an empty store, give the empty answer
    nothing = st.scope([n + 5])
    for kw in ({"scope": nothing}, {"scope": nothing, "per_file": 1}):
        score, cos, ids_, count, flag = st.search_variants_raw(q, k, class_weights=ones, **kw)
        assert count == 0 and not flag and (ids_ == NO_ID).all() and (cos == 0).all() and (score == 0).all()
    assert nothing.route_info()[:2] == (0, 0)  # nothing was launched
    nothing.close()
    sc.close()
    for kw in ({"scope": sc}, {"scope": sc, "per_file": 1}):
        with pytest.raises(_lib.CsError, match="scope is closed"):
            st.search_variants_raw(q, k, class_weights=ones, **kw)
    st.clear()
    st.build_index()
    for kw in ({}, {"per_file": 2}):
        score, cos, ids_, count, flag = st.search_variants_raw(q, k, class_weights=ones, **kw)
        assert count == 0 and not flag and (ids_ == NO_ID).all() and (cos == 0).all() and (score == 0).all()
    foreign.close()
    other.close()
    st.close()
    sharded = VS(None, dim, devices=[0, 0])
    for kw in ({}, {"per_file": 1}):
        with pytest.raises(_lib.CsError, match="sharded store has no boosted search"):
            sharded.search_variants_raw(q, k, class_weights=ones, **kw)
    sharded.close()


def test_two_threads_with_their_own_tables_and_caps(VS):
    n, dim, k = 1000, 384, 25
    rows = synth_rows(9960, 0, n, dim)
    qs = synth_rows(9961, 0, 3, dim)
    st = _store(VS, rows)
    classes = {r: r % 18 for r in range(n)}
    groups = {r: r // 8 for r in range(n)}
    st.set_classes(list(classes), list(classes.values()))
    st.set_groups(list(groups), list(groups.values()))
    truth = [_full_order(st, q) for q in qs]
    half = np.arange(0, n, 2)
    sc = _scope(st, half)
    work_of = [(_kind_weights(3, 1.5), 1, None, None), (_kind_weights(11, 0.25), 3, sc, half)]
    want = [_check(st, _inside(truth, inside), _lookup(classes, NO_CLASS), w, _lookup(groups, NO_GROUP), qs, k, m, s)
            for w, m, s, inside in work_of]
    assert want[0][2].tobytes() != want[1][2].tobytes()
    errors = []

    def work(t):
        w, m, s, _ = work_of[t]
        try:
            for _ in range(20):
                if not _same(st.search_variants_raw(qs, k, class_weights=w, per_file=m, scope=s), want[t]):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    sc.close()
    st.close()
