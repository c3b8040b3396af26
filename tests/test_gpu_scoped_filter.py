"""Scoped searches through the int8 filter (cs_scope_set_route / cs_scope_route_info; plan: codesearch_amd/csrc/
scoped_filter_plan.hpp; launcher: scan_filter.hip scan_split_impl with a prepared plan and the scope's blocked-rows bitmap).

The bar is the scopes' own: whatever the route, a scoped search returns, byte for byte, what the masked search of the same
store returns for a bitmap of exactly the scope's ids — and what the same scope returns on the gathered scan.  Every case
also asserts through route_info() that the route it means to test was the one taken."""
import threading

import numpy as np
import pytest

from codesearch_amd.synth import synth_rows
from tests.test_gpu_scoped_search import _raw_variants, _same

pytestmark = pytest.mark.gpu

SHAPES = [(10, 1), (200, 1), (10, 9), (200, 9), (10, 40)]  # (k, nq)


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows):
    st = VS(None, rows.shape[1])
    st.insert_embeddings(rows)
    st.build_index()
    return st


@pytest.fixture(scope="module")
def store384(VS):
    n, dim = 40_000, 384
    rows = synth_rows(0x5F17, 0, n, dim)
    st = _store(VS, rows)
    qs = np.concatenate([synth_rows(0x5F18, 0, 38, dim), rows[[25_001, n - 3]]])
    yield st, rows, qs
    st.close()


def _masks(n):
    """The scopes of case 1, for a store of n rows."""
    rng = np.random.default_rng(n)
    far = np.arange(n - (3 * n) // 10 - 1000, n - 1000)  # contiguous 30 % in the far half
    # entries 3,072 and 3,073 of the list share a 1,024-row granule, so phase 0 takes more than 3,072 entries
    granule = np.concatenate([np.arange(3000), 5 * 1024 + np.arange(600), np.arange(8192 + 1, n, 3)])
    return {
        "all": np.arange(n),
        "half": np.sort(rng.choice(n, n // 2, replace=False)),
        "every other": np.arange(1, n, 2),
        "far 30 %": far,
        "granule": granule,
    }


def _took(sc, fn):
    """Runs fn() and returns (its result, searches through the filter, gathered searches, overflow reruns) it added."""
    f0, g0, o0, _ = sc.route_info()
    out = fn()
    f1, g1, o1, _ = sc.route_info()
    return out, f1 - f0, g1 - g0, o1 - o0


def _check(st, sc, qs, k, route="filter", want="filter"):
    """The scope's search on `route` took `want`, and equals the masked search and the scope's gathered search."""
    sc.set_route(route)
    a, f, g, over = _took(sc, lambda: st.search_raw(qs, k, scope=sc))
    assert (f, g) == ((1, 0) if want == "filter" else (0, 1)), (route, want, f, g, len(sc), k, qs.shape[0])
    sc.set_route("gather")
    b, f, g, _ = _took(sc, lambda: st.search_raw(qs, k, scope=sc))
    assert (f, g) == (0, 1)
    sc.set_route(route)
    m = st.search_raw(qs, k, chunk_ids=sc.ids)
    assert _same(a, m), ("scoped filter != masked", len(sc), k, qs.shape[0])
    assert _same(a, b), ("scoped filter != scoped gather", len(sc), k, qs.shape[0])
    return a, over


def test_masks_and_shapes_dim_384(store384):
    st, rows, qs = store384
    for name, ids in _masks(40_000).items():
        with st.scope(ids) as sc:
            assert sc.info() == (ids.size, ids.size, 1), name
            assert sc.route_info()[3] >= 40_000 // 8, name  # the bitmap: one bit per stored row
            for k, nq in SHAPES:
                (c, i, cnt), _ = _check(st, sc, qs[:nq], k)
                assert cnt.tolist() == [k] * nq and set(i[0].tolist()) <= set(ids.tolist()), (name, k, nq)


@pytest.mark.parametrize("dim", [768, 1024])
def test_masks_and_shapes_other_dims(VS, dim):
    n = 20_000
    rows = synth_rows(0x5F20 + dim, 0, n, dim)
    st = _store(VS, rows)
    qs = np.concatenate([synth_rows(0x5F21 + dim, 0, 38, dim), rows[[12_001, n - 3]]])
    for name, ids in _masks(n).items():
        with st.scope(ids) as sc:
            for k, nq in SHAPES:
                (c, i, cnt), _ = _check(st, sc, qs[:nq], k)
                assert cnt.tolist() == [k] * nq, (name, k, nq)
    st.close()


def test_auto_route(store384):
    st, rows, qs = store384
    n = 40_000
    with st.scope(_masks(n)["far 30 %"]) as sc:  # dense, in the far half: nine queries take the filter
        _check(st, sc, qs[:9], 10, route="auto", want="filter")
        _check(st, sc, qs[:9], 200, route="auto", want="filter")
        # one query over 12,000 live rows: below the row threshold of a single query
        _check(st, sc, qs[:1], 10, route="auto", want="gather")
    with st.scope(np.concatenate([np.arange(1000, 3000), np.arange(37_000, 39_000)])) as sc:
        # two 5 % blocks of THIS store: phase 0 (3,072 entries and the granule's rest) holds the whole first block, the
        # filter phases stream the second block only, the span is short and AUTO takes the filter
        _check(st, sc, qs[:4], 10, route="auto", want="filter")
    with st.scope(np.arange(0, n, 2)) as sc:  # one query over 20,000 live rows: the row threshold (32,768 below k = 48)
        _check(st, sc, qs[:1], 10, route="auto", want="gather")
        _check(st, sc, qs[:4], 10, route="auto", want="filter")  # always from four queries


def test_auto_route_span_rule(VS):
    """Two far-apart 5 % blocks of a 200,000-row store (large enough that phase 0 ends inside the first block): the
    filter phases would stream the gap too, 8.8 rows per live row.  Four queries may stream 4 (the span rule: gathered),
    nine may stream 10 (filter); the forced route waives the rule."""
    n, dim = 200_000, 384
    st = VS(None, dim)
    st.insert_synthetic(n, 0x5F25, 0)
    st.build_index()
    qs = synth_rows(0x5F26, 0, 9, dim)
    with st.scope(np.concatenate([np.arange(10_000, 20_000), np.arange(180_000, 190_000)])) as sc:
        _check(st, sc, qs[:4], 10, route="auto", want="gather")
        _check(st, sc, qs[:4], 10, route="filter", want="filter")
        _check(st, sc, qs[:9], 10, route="auto", want="filter")
    st.close()


def test_ragged_tail(VS):
    n, dim = 40_037, 384  # 37 rows behind the int8 copy's last complete tile
    rows = synth_rows(0x5F30, 0, n, dim)
    st = _store(VS, rows)
    qs = np.concatenate([synth_rows(0x5F31, 0, 8, dim), rows[[n - 1]]])
    ids = np.concatenate([np.arange(20_000, 39_000, 2), np.arange(39_990, n)])  # the last id is the store's last row
    with st.scope(ids) as sc:
        for k, nq in SHAPES[:4]:
            _check(st, sc, qs[:nq], k)
        (c, i, cnt), _ = _check(st, sc, qs[8:9], 3)
        assert i[0][0] == n - 1  # the store's last row, in the tail, is found through the filter
    with st.scope(np.arange(1, n - 20, 3)) as sc:  # ends inside the tail, before the last row
        _check(st, sc, qs[:9], 10)
    st.close()


def test_ties_keep_id_order(VS):
    n, dim = 40_000, 384
    rows = synth_rows(0x5F40, 0, n, dim)
    q = synth_rows(0x5F41, 0, 1, dim)
    rows[[100, 20_100, 39_900]] = q[0]
    st = _store(VS, rows)
    with st.scope(np.arange(10_000, n)) as sc:  # 100 is not in it
        (c, i, cnt), _ = _check(st, sc, q, 2)
        assert i[0].tolist() == [20_100, 39_900] and c[0][0] == c[0][1]
        (c, i, cnt), _ = _check(st, sc, np.repeat(q, 9, axis=0), 2)
        assert (i == np.array([20_100, 39_900])).all()
    st.close()


def test_tombstones_and_reclaim(VS):
    n, dim, k = 40_000, 384, 50
    rows = synth_rows(0x5F50, 0, n, dim)
    st = _store(VS, rows)
    rng = np.random.default_rng(50)
    ids = np.sort(rng.choice(n, n // 2, replace=False))
    qs = np.concatenate([synth_rows(0x5F51, 0, 7, dim), rows[ids[[5, -5]]]])
    sc = st.scope(ids)
    _check(st, sc, qs, k)
    assert sc.info() == (ids.size, ids.size, 1)
    # tombstones only: 5 % of the scope's ids, 2.5 % of the rows
    dead = np.sort(rng.choice(ids, ids.size // 20, replace=False))
    st.delete_chunks(dead.tolist())
    st.build_index()
    assert st.stored_rows() == n
    (c, i, cnt), _ = _check(st, sc, np.concatenate([qs, rows[dead[:2]]]), k)
    assert not (set(i.ravel().tolist()) & set(dead.tolist()))
    assert sc.info() == (ids.size, ids.size - dead.size, 2)
    # a reclaiming build (15 % of the scope's ids more: 10 % of the rows are tombstones): rows move, the row -> id table exists
    more = np.sort(rng.choice(np.setdiff1d(ids, dead), (ids.size * 3) // 20, replace=False))
    st.delete_chunks(more.tolist())
    st.build_index()
    assert st.stored_rows() == n - dead.size - more.size
    (c, i, cnt), _ = _check(st, sc, np.concatenate([qs, rows[more[:2]]]), k)
    assert not (set(i.ravel().tolist()) & (set(dead.tolist()) | set(more.tolist())))
    assert sc.info() == (ids.size, ids.size - dead.size - more.size, 3)
    _check(st, sc, qs[:1], 10)
    assert sc.info()[2] == 3  # the same generation: no refresh
    sc.close()
    st.close()


def test_overflow_is_settled_by_the_scope_own_rerun(VS):
    """Rows ordered so that the cosine to the query rises with the row index: every allowed row of a phase beats the
    running k-th best, so the phase behind phase 0 appends one candidate per allowed row — more than a candidate buffer
    holds (settle_overflow's "adversarial row order").  The exact rerun over the scope's list answers."""
    n, dim = 40_000, 384
    noise = synth_rows(0x5F60, 0, n, dim).astype(np.float64)
    q = synth_rows(0x5F61, 0, 1, dim).astype(np.float64)[0]
    q /= np.linalg.norm(q)
    noise -= np.outer(noise @ q, q)
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cos = np.linspace(0.0, 0.5, n)
    rows = (cos[:, None] * q[None, :] + np.sqrt(1.0 - cos * cos)[:, None] * noise).astype(np.float32)
    st = _store(VS, rows)
    assert st.filter_state()[0] == 2  # the int8 copy serves
    qs = q[None, :].astype(np.float32)
    with st.scope(np.arange(1, n, 2)) as sc:
        (c, i, cnt), over = _check(st, sc, qs, 10)
        assert over >= 1 and sc.route_info()[2] >= 1
        assert i[0].tolist() == list(range(n - 1, n - 21, -2))
        assert st.filter_state()[0] == 2  # no strike retired the index's int8 copy
        # ... nor later: overflow once more, then unscoped multi-query searches on this thread (the same pooled
        # workspace: their first kernel folds what a search left in the overflow word into the device's count, and the
        # search after that would turn it into a strike; two strikes among so few int8 searches retire the copy)
        counters = st.debug_counters()
        _, over = _check(st, sc, qs, 10)
        assert over >= 1
        many = synth_rows(0x5F62, 0, 6, dim).astype(np.float64)
        many = (many - np.outer(many @ q, q)).astype(np.float32)  # orthogonal to q: no trend along the rows for them
        for _ in range(4):
            st.search_raw(many, 10)
            assert st.filter_state()[0] == 2
        _, over = _check(st, sc, qs, 10)
        assert over >= 1
        for _ in range(4):
            st.search_raw(many, 10)
        assert st.filter_state()[0] == 2
        # the scope's overflows are counted per scope, not in the index's batched fallbacks
        assert st.debug_counters() == (counters[0] + 8, counters[1])
    st.close()


def test_scopes_that_never_take_the_filter(VS, store384):
    st, rows, qs = store384
    with st.scope(np.arange(5000, 6000)) as sc:  # too small for a bitmap
        assert sc.route_info() == (0, 0, 0, 0)
        _check(st, sc, qs[:9], 10, route="filter", want="gather")
        assert sc.route_info()[0] == 0 and sc.route_info()[3] == 0
    n, dim = 20_000, 100
    r100 = synth_rows(0x5F70, 0, n, dim)
    s100 = _store(VS, r100)
    with s100.scope(np.arange(0, n, 2)) as sc:
        _check(s100, sc, synth_rows(0x5F71, 0, 9, dim), 10, route="filter", want="gather")
        assert sc.route_info()[0] == 0 and sc.route_info()[3] == 0
    s100.close()


def test_variants_form(store384):
    st, rows, _ = store384
    ids = _masks(40_000)["half"]
    near = rows[ids[11]]
    qs = np.stack([near + 0.01 * synth_rows(0x5F80 + v, 0, 1, 384)[0] for v in range(9)]).astype(np.float32)
    far = synth_rows(0x5F90, 0, 9, 384)
    with st.scope(ids) as sc:
        sc.set_route("filter")
        for q in (qs, far, qs[:1]):
            for k in (200, 10):
                a, f, g, _ = _took(sc, lambda: _raw_variants(st, q, k, scope=sc))
                assert (f, g) == (1, 0)
                sc.set_route("gather")
                b, f, g, _ = _took(sc, lambda: _raw_variants(st, q, k, scope=sc))
                assert (f, g) == (0, 1)
                sc.set_route("filter")
                assert a == b and a == _raw_variants(st, q, k, chunk_ids=ids)
        assert _raw_variants(st, qs, 200, scope=sc)[2] == 200


def test_threads_scopes_and_routes(store384):
    st, rows, qs = store384
    masks = [_masks(40_000)["half"], _masks(40_000)["far 30 %"]]
    scopes = [st.scope(m) for m in masks]
    scopes[0].set_route("filter")
    scopes[1].set_route("auto")
    jobs = [(0, 1, 10), (0, 9, 200), (1, 9, 10), (1, 1, 200)]  # (scope, nq, k) per thread
    want = [st.search_raw(qs[:nq], k, chunk_ids=masks[s]) for s, nq, k in jobs]
    for (s, nq, k), w in zip(jobs, want):
        assert _same(st.search_raw(qs[:nq], k, scope=scopes[s]), w)
    errors = []

    def work(t):
        s, nq, k = jobs[t]
        try:
            for _ in range(8):
                if not _same(st.search_raw(qs[:nq], k, scope=scopes[s]), want[t]):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    f0, g0, _, _ = scopes[0].route_info()
    f1, g1, _, _ = scopes[1].route_info()
    assert (f0, g0) == (18, 0) and (f1, g1) == (9, 9)  # the far scope: nine queries filter, one query gathers
    for sc in scopes:
        sc.close()
