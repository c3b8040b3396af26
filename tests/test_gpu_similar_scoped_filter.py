"""Similar-chunk search inside a scope through the int8 filter (cs_index_search_similar_scoped on a scope whose route takes
the filter: index.hip run_similar_scoped, scan_filter.hip scan_split_impl with a prepared plan AND a SimilarRefine, the list
form of scan_similar_filter.hip similar_rescore_kernel in phase 0).

The truth is code that exists without the feature: the same call with the scope on its GATHER route — the gathered f32 scan
under the exclusions, which tests/test_gpu_similar_scoped.py pins to the host reducer.  The bar of every case is the same:
identical bytes of cosines, ids and counts between the two routes, and route_info() showing that the filter answered
(filter_searches + 1, gathered_searches + 0).

Stores are synth_rows with ids in files of 8 and an ungrouped tail; in the large store every 50th file (file % 50 == 2) is a
file of near-duplicates of its first row, so that a file exclusion that is not applied, in phase 0 or behind it, shows in
the returned ids.  The phase plans named in the docstrings were checked on the CPU with plan_scoped_filter and
scoped_wants_filter (256 CUs, the default knobs)."""
import itertools
import threading

import numpy as np
import pytest

from codesearch_amd.search import NO_GROUP
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

MODES = ("none", "self", "file")
SHAPES = [(10, 1), (200, 1), (10, 9), (200, 9), (10, 40)]  # (k, nq); 40 > 32 queries: phase 0 is 1,024 entries
UNGROUPED = 40


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _planted(rows, seed):
    """Every 50th file of 8 (file % 50 == 2, not in the ungrouped tail) becomes near-duplicates of its first row."""
    n = len(rows)
    noise = synth_rows(seed, 0, n, rows.shape[1])
    for f in range(2, (n - UNGROUPED) // 8, 50):
        rows[8 * f + 1:8 * f + 8] = 0.9 * rows[8 * f] + 0.1 * noise[8 * f + 1:8 * f + 8]
    return rows


def _store(VS, rows, id_base=0):
    """rows in a built store, ids in files of 8 with an ungrouped tail."""
    st = VS(None, rows.shape[1], id_base=id_base)
    st.insert_embeddings(rows)
    st.build_index()
    g = len(rows) - UNGROUPED
    st.set_groups(np.arange(g) + id_base, np.arange(g) // 8)
    return st


@pytest.fixture(scope="module")
def store384(VS):
    n, dim = 40_000, 384
    rows = _planted(synth_rows(0x51F0, 0, n, dim), 0x51F1)
    st = _store(VS, rows)
    assert st.filter_state()[0] == 2  # the int8 copy serves
    yield st, rows
    st.close()


def _masks(n):
    """The scopes of tests/test_gpu_scoped_filter.py::_masks, for a store of n rows."""
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


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _took(sc, fn):
    """Runs fn() and returns (its result, searches through the filter, gathered searches, overflow reruns) it added."""
    f0, g0, o0, _ = sc.route_info()
    out = fn()
    f1, g1, o1, _ = sc.route_info()
    return out, f1 - f0, g1 - g0, o1 - o0


def _both(st, sc, srcs, k, mode, min_cos=None, route="filter", want="filter"):
    """The call on the scope's `route` took `want` and equals, byte for byte, the call on GATHER. -> (answer, overflow reruns)"""
    call = lambda: st.similar_raw(srcs, k, exclude=mode, min_cos=min_cos, scope=sc)
    sc.set_route(route)
    a, f, g, over = _took(sc, call)
    assert (f, g) == ((1, 0) if want == "filter" else (0, 1)), (route, want, f, g, len(sc), len(srcs), k, mode)
    sc.set_route("gather")
    b, f, g, _ = _took(sc, call)
    assert (f, g) == (0, 1)
    sc.set_route(route)
    for name, x, y in zip(("cos", "ids", "counts"), a, b):
        assert x.tobytes() == y.tobytes(), (name, len(sc), len(srcs), k, mode, min_cos)
    return a, over


def _planted_in(ids, n):
    """The scope's ids that lie in a planted file, ascending."""
    ids = np.asarray(ids)
    return ids[((ids // 8) % 50 == 2) & (ids < n - UNGROUPED)]


def _sources(ids, n, nq):
    """nq sources for the scope `ids` of a store of n rows.  The first is a planted-file row among the list's first entries
    (phase 0's exclusions, the list form), then a row of the SAME file (two sources of one file in one query tile; in the
    scope or not), a planted-file row far behind phase 0, an ungrouped source (the last id), the first one again (a
    duplicate), an id outside the scope (if there is one), then a spread over the store."""
    p = _planted_in(ids, n)
    first, last = int(p[0]), int(p[-1])
    pos = {int(v): i for i, v in enumerate(np.asarray(ids)[:1024].tolist())}
    assert first in pos and int(np.searchsorted(ids, last)) > 4096  # inside every phase 0 / behind every phase 0
    outside = np.setdiff1d(np.arange(n), ids)
    head = [first, first ^ 1, last, n - 1, first] + ([int(outside[len(outside) // 2])] if outside.size else []) + [last ^ 1, 100, 8]
    tail = [(i * 7919 + 13) % n for i in range(nq)]
    order = {1: [first], 2: [last, first]}.get(nq, head + tail)
    return order[:nq]


def _file_of(i):
    return set(range(i // 8 * 8, i // 8 * 8 + 8))


def test_masks_and_shapes_dim_384(store384):
    """Phase 0 of "all" is entries = rows [0, 3,072) (1,024 at 40 queries); of "granule" c0 > 3,072; of "far 30 %" 3,720
    entries that end at row 30,720."""
    st, rows = store384
    n = 40_000
    for name, ids in _masks(n).items():
        mates = set(ids.tolist())
        with st.scope(ids) as sc:
            for (k, nq), mode in itertools.product(SHAPES, MODES):
                srcs = _sources(ids, n, nq)
                (cos, got, cnt), over = _both(st, sc, srcs, k, mode)
                assert over == 0 and (cnt == k).all(), (name, k, nq, mode)
                assert set(got.ravel().tolist()) <= mates, (name, k, nq, mode)
                for q, s in enumerate(srcs):  # the exclusions show: every source here but the spread has near-duplicates
                    file_in_scope = (_file_of(s) & mates) if s < n - UNGROUPED else set()
                    hits = set(got[q].tolist())
                    if mode == "file":
                        assert not hits & (file_in_scope | {s}), (name, k, nq, q, s)
                    elif (s // 8) % 50 == 2 and s < n - UNGROUPED:
                        assert file_in_scope - {s} <= hits, (name, k, nq, mode, q, s)
                        assert (s in hits) == (mode == "none" and s in mates)
            # one source behind phase 0, alone and first in its tile
            p = _planted_in(ids, n)
            for mode in MODES:
                (cos, got, cnt), _ = _both(st, sc, [int(p[-1])], 10, mode)
                assert (int(p[-1]) in got[0].tolist()) == (mode == "none")
                if mode == "file":
                    assert not set(got[0].tolist()) & _file_of(int(p[-1]))


def test_identities(store384):
    st, rows = store384
    n, k = 40_000, 10
    srcs = _sources(np.arange(n), n, 9)
    with st.scope(np.arange(n)) as sc:  # a scope of every id equals the unscoped call, on either similar route
        for mode, bound in itertools.product(MODES, (None, 0.1)):
            (a, _) = _both(st, sc, srcs, k, mode, min_cos=bound)
            for route in ("scan", "filter"):
                st.set_similar_route(route)
                assert _same(a, st.similar_raw(srcs, k, exclude=mode, min_cos=bound)), (mode, bound, route)
        st.set_similar_route("auto")
    ids = _masks(n)["every other"]
    with st.scope(ids) as sc:
        # "none" with no bound is the ordinary scoped search of the source's stored row
        srcs = _sources(ids, n, 9)
        for kk in (10, 200):
            a, _ = _both(st, sc, srcs, kk, "none")
            q = np.concatenate([st.read_rows(s, 1) for s in srcs])
            for route in ("filter", "gather"):
                sc.set_route(route)
                assert _same(a, st.search_raw(q, kk, scope=sc)), (kk, route)
        # "self" with a source outside the scope (even ids) equals "none"
        out = [16, 18, 5000, 39_000, 16]
        a, _ = _both(st, sc, out, k, "self")
        b, _ = _both(st, sc, out, k, "none")
        assert _same(a, b)


@pytest.mark.parametrize("dim", [768, 1024])
def test_other_dims(VS, dim):
    """20,000 rows, every other id: phase 0 = the list's first 3,072 entries = rows [0, 6,144), one filter phase
    [6,144, 20,000)."""
    n = 20_000
    st = _store(VS, _planted(synth_rows(0x5200 + dim, 0, n, dim), 0x5201 + dim))
    ids = np.arange(1, n, 2)
    with st.scope(ids) as sc:
        for (k, nq), mode in itertools.product(SHAPES[:4], MODES):
            (cos, got, cnt), over = _both(st, sc, _sources(ids, n, nq), k, mode)
            assert over == 0 and (cnt == k).all()
    st.close()


def test_ragged_tail(VS):
    n, dim = 40_037, 384  # 37 rows behind the int8 copy's last complete tile
    rows = _planted(synth_rows(0x5210, 0, n, dim), 0x5211)
    rows[n - 1] = 0.9 * rows[20_010] + 0.1 * rows[n - 1]  # a near-duplicate of a source in the store's last row
    st = _store(VS, rows)
    ids = np.concatenate([np.arange(20_000, 39_000, 2), np.arange(39_990, n)])  # ends in the store's last row
    with st.scope(ids) as sc:
        for (k, nq), mode in itertools.product(SHAPES[:4], MODES):
            _both(st, sc, ([20_010, n - 1, 38_000, 5] + _sources(ids, n, 9))[:nq], k, mode)
        for mode in MODES:
            (cos, got, cnt), _ = _both(st, sc, [20_010, n - 1], 3, mode)
            assert got[0][0 if mode != "none" else 1] == n - 1  # the last row, in the tail, is found through the filter
            assert got[1][0 if mode != "none" else 1] == 20_010  # ... and is a source
    ids = np.arange(1, n - 20, 3)  # ends inside the 37-row tail, before the last row
    with st.scope(ids) as sc:
        assert ids[-1] >= n - 37
        for mode in MODES:
            _both(st, sc, _sources(ids, n, 9), 10, mode)
            _both(st, sc, [int(ids[-1]), n - 1], 10, mode)
    st.close()


def test_min_cos_is_a_strict_bound(store384):
    st, rows = store384
    n, k = 40_000, 10
    ids = _masks(n)["half"]
    srcs = [100] + _sources(ids, n, 8)
    with st.scope(ids) as sc:
        for mode in MODES:
            sc.set_route("gather")
            cos, got, cnt = st.similar_raw(srcs, k, exclude=mode, scope=sc)
            fifth = float(cos[0][4])  # the cosine the gathered scan returned at rank 5 for the first source
            assert cos[0][3] > cos[0][4]
            a, _ = _both(st, sc, srcs, k, mode, min_cos=fifth)
            assert a[2][0] == 4 and a[1][0][:4].tobytes() == got[0][:4].tobytes()  # strict: that row and all under it are gone
            assert fifth not in a[0][0][:4].tolist()
            for bound in (0.0, 0.1, 0.5):
                _both(st, sc, srcs, k, mode, min_cos=bound)
            # a bound above every cosine: nothing, and no overflow — the fold's floor keeps tau at the bound
            a, over = _both(st, sc, srcs, k, mode, min_cos=2.0)
            assert (a[2] == 0).all() and (a[1] == 0xFFFFFFFF).all() and (a[0] == 0).all() and over == 0
            # ... also where the bound leaves fewer than k rows but some (a list that never fills)
            a, over = _both(st, sc, srcs, 200, mode, min_cos=0.15)
            assert 0 < int(a[2].max()) < 200 and over == 0
        assert sc.route_info()[2] == 0


def test_ties_go_to_the_lower_id(VS):
    n, k = 20_000, 10
    rows = synth_rows(0x5220, 0, n, 384)
    rows[5] = rows[7001]     # a twin with a lower id inside phase 0, the source behind it
    rows[15_001] = rows[41]  # a twin with a higher id behind phase 0, the source inside it
    st = _store(VS, rows)
    srcs = [7001, 5, 41, 15_001, 123]
    with st.scope(np.arange(1, n, 2)) as sc:  # phase 0 = rows [0, 6,144)
        none, _ = _both(st, sc, srcs, k, "none")
        assert none[1][0][:2].tolist() == [5, 7001] and none[1][1][:2].tolist() == [5, 7001]
        assert none[1][2][:2].tolist() == [41, 15_001] and none[1][3][:2].tolist() == [41, 15_001]
        assert none[0][0][0].tobytes() == none[0][0][1].tobytes() and none[0][2][0].tobytes() == none[0][2][1].tobytes()
        self_, _ = _both(st, sc, srcs, k, "self")
        assert self_[1][:4, 0].tolist() == [5, 7001, 15_001, 41]  # SELF returns the twin
        _both(st, sc, srcs, k, "file")
    st.close()


def test_life_cycle_tombstones_and_a_reclaiming_build(VS):
    n, base, k = 20_000, 7000, 10
    st = _store(VS, _planted(synth_rows(0x5230, 0, n, 384), 0x5231), id_base=base)
    srcs = [base + r for r in (17, 16, 5001, 12_345, n - 1, 17, 3071, 6145, 19_217)]
    sc = st.scope(base + np.arange(1, n, 2))  # phase 0 = rows [0, 6,144) while nothing is deleted
    for mode in MODES:
        _both(st, sc, srcs, k, mode)
    assert sc.info()[2] == 1
    # tombstones inside phase 0 and behind it, among them the first and the last source's nearest neighbours; no reclaim yet
    sc.set_route("gather")
    near = [int(i) for i in st.similar_raw([srcs[0], srcs[-1]], 6, exclude="self", scope=sc)[1].ravel()]
    first = sorted((set(near) | {base + r for r in range(3, n, 23)}) - set(srcs))
    assert len(first) * 10 < n and any(i < base + 6144 for i in near) and any(i >= base + 6144 for i in near)
    assert st.delete_chunks(first) == len(first)
    st.build_index()
    assert st.stored_rows() == n and len(st) == n - len(first)
    for mode in MODES:
        for kk in (k, 200):
            got, _ = _both(st, sc, srcs, kk, mode)
            assert not set(got[1].ravel().tolist()) & set(first)
    assert sc.info()[2] == 2
    # 30 % deleted in all: the build reclaims, every surviving row behind the first hole moves, the scope's list is remade
    pool = [base + r for r in range(n) if base + r not in set(srcs) and base + r not in set(first)]
    more = sorted(pool, key=lambda i: ((i - base) % 10 not in (0, 1, 5), i))[:(3 * n) // 10 - len(first)]
    assert st.delete_chunks(more) == len(more)
    st.build_index()
    gone = set(first) | set(more)
    assert st.stored_rows() == len(st) == n - len(gone)
    for mode in MODES:
        for kk in (k, 200):
            got, _ = _both(st, sc, srcs, kk, mode)  # sources the build moved
            assert not set(got[1].ravel().tolist()) & gone
    assert sc.info()[2] == 3 and sc.info()[1] > 3072 + 1024
    _both(st, sc, srcs, k, "file", min_cos=0.1)
    assert sc.route_info()[2] == 0
    sc.close()
    st.close()


def test_an_excluded_hog_overflows_and_the_gathered_similar_scan_answers(VS):
    """The store of tests/test_gpu_similar_filter.py::test_an_excluded_hog_overflows_and_the_scan_answers: rows 8,000-13,999
    are near-duplicates (cosine >= 0.95) of row 8,000 and form one group.  The scope is the ids 4,000-19,999, the source
    8,000, the mode "file", k = 10.  The plan: c0 = 3,168, phase 0 = rows [0, 7,168), one filter phase [7,168, 20,000) that
    holds all 5,999 excluded near-duplicates — more than the 4,096 candidates the buffer holds.  The scope's gathered similar
    scan answers; nothing of the index's bookkeeping moves."""
    n, dim, k, src = 20_000, 384, 10, 8000
    noise = synth_rows(9900, 0, n, dim)
    rows = noise.copy()
    hog = np.arange(8000, 14_000)
    rows[hog[1:]] = 0.95 * rows[src] + 0.05 * noise[hog[1:]]
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    assert float((unit[hog] @ unit[src]).min()) >= 0.95
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    groups[hog] = 0
    groups[n - UNGROUPED:] = NO_GROUP
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    st.set_groups(np.arange(n), groups)
    assert st.filter_state()[0] == 2
    queries = synth_rows(9901, 0, 4, dim)
    sc = st.scope(np.arange(4000, n))
    state0, counters0, similar0 = st.filter_state(), st.debug_counters(), st.similar_route_info()
    for rep in range(3):
        state, counters = st.filter_state(), st.debug_counters()
        got, over = _both(st, sc, [src], k, "file")  # filter_searches + 1 (asserted there)
        assert over == 1
        assert st.filter_state() == state and st.debug_counters() == counters
        assert got[2][0] == k and not (groups[got[1][0]] == 0).any() and (got[1][0] >= 4000).all()
        for _ in range(2):  # ordinary searches through the same pooled workspace: none is struck for the scope's overflow
            c, i, cnt = st.search_raw(queries, k)
            assert (cnt == k).all()
    assert st.filter_state() == state0 and state0[0] == 2
    assert st.debug_counters() == (counters0[0] + 6, counters0[1])
    assert st.similar_route_info() == similar0
    assert sc.route_info()[:3] == (3, 3, 3)
    _both(st, sc, [16, 17, 100, n - 1, 16, 23, 8, 7], k, "file")  # ordinary sources, none of the hog
    sc.close()
    st.close()


def test_routes(VS, store384):
    st, rows = store384
    n, k = 40_000, 10
    ids = _masks(n)["every other"]
    with st.scope(ids) as sc:
        # AUTO follows scoped_wants_filter: 20,000 live rows take the filter from two sources on, one source gathers
        # (the row threshold of a single query)
        for nq, want in ((1, "gather"), (2, "filter"), (9, "filter"), (40, "filter")):
            _both(st, sc, _sources(ids, n, nq), k, "file", route="auto", want=want)
        # ... as the ordinary scoped search of as many queries does
        for nq, took in ((1, (0, 1)), (9, (1, 0))):
            _, f, g, _ = _took(sc, lambda: st.search_raw(rows[:nq], k, scope=sc))
            assert (f, g) == took
        # GATHER never takes the filter; the unscoped call's route does not govern, its counters do not move
        before = st.similar_route_info()
        for route in ("scan", "filter", "auto"):
            st.set_similar_route(route)
            _both(st, sc, _sources(ids, n, 9), k, "self", route="gather", want="gather")
            _both(st, sc, _sources(ids, n, 9), k, "self", route="filter", want="filter")
        assert st.similar_route_info() == before
    # FILTER quietly gathers on a scope that fits phase 0 and on a dim without filter kernels
    with st.scope(np.arange(5000, 6000)) as sc:
        for mode in MODES:
            _both(st, sc, [16, 5016, 5017], k, mode, route="filter", want="gather")
        assert sc.route_info()[0] == 0 and sc.route_info()[3] == 0
    n100 = 20_000
    s100 = _store(VS, synth_rows(0x5240, 0, n100, 100))
    with s100.scope(np.arange(0, n100, 2)) as sc:
        for mode in MODES:
            _both(s100, sc, [16, 17, 100, n100 - 1, 16, 23, 0, 7, 8], k, mode, route="filter", want="gather")
        assert sc.route_info()[0] == 0
    s100.close()


def test_concurrent_calls_on_the_filter_route(store384):
    st, rows = store384
    n, k = 40_000, 25
    masks = [_masks(n)["half"], _masks(n)["far 30 %"]]
    scopes = [st.scope(m) for m in masks]
    rng = np.random.default_rng(13)
    jobs = [(rng.integers(0, n, nq).tolist(), mode, bound, s) for nq, mode, bound, s in
            [(1, "self", None, 0), (3, "file", None, 1), (9, "none", 0.0, 0), (40, "file", 0.05, 1)]]
    for sc in scopes:
        sc.set_route("gather")
    want = [st.similar_raw(s, k, exclude=m, min_cos=b, scope=scopes[i]) for s, m, b, i in jobs]
    assert all(int(w[2].max()) > 0 for w in want)
    for sc in scopes:
        sc.set_route("filter")
    before = [sc.route_info()[:3] for sc in scopes]
    errors = []

    def work(t):
        try:
            s, m, b, i = jobs[t]
            for _ in range(20):
                if not _same(st.similar_raw(s, k, exclude=m, min_cos=b, scope=scopes[i]), want[t]):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    for sc, b in zip(scopes, before):
        assert sc.route_info()[:3] == (b[0] + 40, b[1], b[2])
        sc.close()
