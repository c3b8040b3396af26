"""Grouped variants search (cs_index_search_variants_grouped / _grouped_scoped, codesearch_amd/csrc/scan_grouped.hip: capped
per-variant lists, then merge_variants_grouped_kernel): a row's key is the best of its keys over the query variants, the
rows are ordered by it and capped per group.

Ground truth comes only from code that exists without the feature: every variant's full order of the rows in play —
search_raw(variant, n) on the streaming route, or search_raw(variant, n, scope=...) on the gathered one, at most 1,024
rows, with its cosine bits — merged and capped on the host by search.merge_variants_capped; the flag is
search.high_confidence of the expected list.  Ids must match exactly, cosines, count and flag bit for bit."""
import numpy as np
import pytest

from codesearch_amd.search import NO_GROUP, high_confidence, merge_variants_capped
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows):
    st = VS(None, rows.shape[1])
    st.insert_embeddings(rows)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    return st


def _variants(q, nv, seed):
    """The query plus small noise, so ids recur with other cosines; from two variants on, the last is an exact copy of the
    first."""
    noise = synth_rows(seed, 0, nv, q.shape[0])
    v = np.stack([q + 0.15 * np.linalg.norm(q) / np.linalg.norm(noise[j]) * noise[j] for j in range(nv)]).astype(np.float32)
    v[0] = q
    if nv >= 2:
        v[-1] = v[0]
    return v


def _full_orders(st, vs, n, sc=None):
    """Per variant the full order (cos, ids) of the n rows in play: one query per call, so the streaming route."""
    out = []
    for v in vs:
        c, i, cnt = st.search_raw(v, n, scope=sc) if sc is not None else st.search_raw(v, n)
        assert cnt[0] == n
        out.append((c[0].copy(), i[0].copy()))
    return out


def _check(st, lists, lookup, vs, k, m, sc=None):
    cos, ids, count, flag = st.search_variants_raw(vs, k, scope=sc, per_file=m)
    ec, ei = merge_variants_capped(lists, lookup, k, m)
    n = len(ei)
    assert count == n, (k, m, count, n)
    assert ids[:n].tolist() == ei, (k, m)
    assert cos[:n].tobytes() == np.asarray(ec, np.float32).tobytes(), (k, m)
    assert (ids[n:] == NO_ID).all() and (cos[n:] == 0).all()
    assert flag == high_confidence(ec), (k, m, flag)
    return ei


@pytest.mark.parametrize("scoped", [False, True])
@pytest.mark.parametrize("dim", [384, 100])
def test_grouped_variants_equal_the_capped_merge_of_full_orders(VS, dim, scoped):
    n, seed = 1000, 9600 + dim
    rows = synth_rows(seed, 0, n, dim)
    q = synth_rows(seed + 1, 0, 1, dim)[0]
    st = _store(VS, rows)
    sc = None
    n_play = n
    if scoped:
        sc = st.scope(np.arange(0, n, 3))  # every third id
        sc.set_route("gather")
        n_play = len(sc)
    orders = {}
    for nv in (1, 2, 9):
        vs = _variants(q, nv, seed + 10 + nv)
        orders[nv] = (vs, _full_orders(st, vs, n_play, sc))
    groupings = [("none", {}), ("mod7", {r: r % 7 for r in range(n)}), ("files16", {r: r // 16 for r in range(n)}),
                 ("one", {r: 3 for r in range(n)})]
    for _name, groups in groupings:
        if groups:
            st.set_groups(list(groups), list(groups.values()))
        lookup = lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]
        for nv, (vs, lists) in orders.items():
            for k in (10, 200, 1000):  # nine lists of 1,000 keys: the merge takes two levels
                for m in (1, 3):
                    _check(st, lists, lookup, vs, k, m, sc)
    # a variant that is an exact copy changes nothing
    vs, lists = orders[9]
    a = st.search_variants_raw(vs, 200, scope=sc, per_file=3)
    b = st.search_variants_raw(vs[:-1], 200, scope=sc, per_file=3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]
    if sc is not None:
        sc.close()
    st.close()


def test_the_flag_is_the_predicate_on_the_capped_list(VS):
    n, dim = 1000, 384
    rows = synth_rows(641, 0, n, dim)
    q = synth_rows(642, 0, 1, dim)[0]
    twins = [100, 200, 300, 400, 500]
    rows[twins] = q
    st = _store(VS, rows)
    vs = _variants(q, 3, 643)
    lists = _full_orders(st, vs, n)
    # five rows equal to the query, in five different groups: all five lead the capped list
    groups = {r: r for r in range(n)}
    st.set_groups(list(groups), list(groups.values()))
    cos, ids, count, flag = st.search_variants_raw(vs, 10, per_file=1)
    assert flag and ids[:5].tolist() == twins
    _check(st, lists, lambda i: [groups[int(x)] for x in i], vs, 10, 1)
    # the same five rows in one group: the uncapped variants search is confident, the capped list keeps one of them
    groups.update({r: 7000 for r in twins})
    st.set_groups(list(groups), list(groups.values()))
    assert st.search_variants_raw(vs, 10)[3] is True
    cos, ids, count, flag = st.search_variants_raw(vs, 10, per_file=1)
    assert not flag and count == 10 and ids[0] == twins[0] and not set(ids[1:].tolist()) & set(twins)
    _check(st, lists, lambda i: [groups[int(x)] for x in i], vs, 10, 1)
    with st.scope(np.arange(n)) as sc:  # ... and through a scope
        assert st.search_variants_raw(vs, 10, scope=sc)[3] is True
        assert st.search_variants_raw(vs, 10, scope=sc, per_file=1)[3] is False
    st.close()


@pytest.mark.parametrize("dim", [384, 100])
def test_uncapped_equals_the_variants_search(VS, dim):
    """per_file >= k, and no group assigned: cs_index_search_variants / _variants_scoped on every returned field."""
    n = 1000
    rows = synth_rows(9650 + dim, 0, n, dim)
    q = rows[17] + 0.5 * synth_rows(9651 + dim, 0, 1, dim)[0]
    st = _store(VS, rows)
    sc = st.scope(np.arange(0, n, 3))
    sc.set_route("gather")

    def same(a, b):
        return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]

    for nv in (1, 2, 9):
        vs = _variants(q, nv, 9652 + dim + nv)
        for k in (10, 200, 1000):
            for kw in ({}, {"scope": sc}):
                want = st.search_variants_raw(vs, k, **kw)
                assert same(st.search_variants_raw(vs, k, per_file=1, **kw), want)  # no group assigned
                st.set_groups(np.arange(n), np.arange(n) % 4)
                assert not same(st.search_variants_raw(vs, k, per_file=1, **kw), want)  # (four groups: the cap bites)
                for m in (k, 0xFFFFFFFF):
                    assert same(st.search_variants_raw(vs, k, per_file=m, **kw), want), (nv, k, m, kw)
                st.set_groups(np.arange(n), np.full(n, NO_GROUP))
    sc.close()
    st.close()
