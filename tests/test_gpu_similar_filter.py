"""Similar-chunk search through the filter (cs_index_set_similar_route, codesearch_amd/csrc/scan_similar_filter.hip): the
int8 / f16 filter of the ordinary search with a refine that drops the excluded rows and the rows under the bound, and a fold
whose threshold never falls below the bound.

The truth is code that exists without the feature: the same call on set_similar_route("scan") — the f32 streaming scan under
the exclusions, which tests/test_gpu_similar_search.py pins to the host reducer and the oracle.  The criterion is identical
bytes of cosines, ids and counts between the two routes, and similar_route_info() showing which route answered."""
import itertools
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, drop_excluded
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

MODES = ("none", "self", "file")
NQS = (1, 2, 9, 40, 130)  # 130: past one 128-query tile
KS = (1, 10, 200)


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows, id_base=0, ungrouped=40):
    """rows in a built store, ids in files of 8 with an ungrouped tail."""
    st = VS(None, rows.shape[1], id_base=id_base)
    st.insert_embeddings(rows)
    st.build_index()
    n = len(rows)
    g = max(n - ungrouped, 0)
    if g:
        st.set_groups(np.arange(g) + id_base, np.arange(g) // 8)
    return st


def _sources(n, nq, base=0):
    """nq source ids of a store of n rows: two sources of one file in the first query tile (16, 17), an ungrouped one (the
    last id), a duplicate (16 again), then a spread."""
    head = [16, 17, 100, n - 1, 16, 23, 0, 7, 8]
    tail = [(i * 7919 + 13) % n for i in range(nq)]
    return [base + (s % n) for s in (head + tail)[:nq]]


def _both(st, srcs, k, mode, min_cos=None, route="filter", filtered=True, fallbacks=0):
    """The call on the scan route and on `route`; bytes equal; the counters say which route answered. -> the answer."""
    st.set_similar_route("scan")
    s0 = st.similar_route_info()
    want = st.similar_raw(srcs, k, exclude=mode, min_cos=min_cos)
    s1 = st.similar_route_info()
    assert s1 == (s0[0], s0[1] + 1, s0[2])
    st.set_similar_route(route)
    got = st.similar_raw(srcs, k, exclude=mode, min_cos=min_cos)
    s2 = st.similar_route_info()
    for name, x, y in zip(("cos", "ids", "counts"), got, want):
        assert x.tobytes() == y.tobytes(), (name, len(st), len(srcs), k, mode, min_cos)
    if filtered:
        assert s2 == (s1[0] + 1, s1[1], s1[2] + fallbacks), (s1, s2, len(st), len(srcs), k, mode)
    else:
        assert s2 == (s1[0], s1[1] + 1, s1[2]), (s1, s2)
    return got


def _matrix(st, n, ks=KS, nqs=NQS, base=0):
    for nq, k, mode in itertools.product(nqs, ks, MODES):
        _both(st, _sources(n, nq, base), k, mode)


@pytest.mark.parametrize("n", [1, 2, 127, 1000])
def test_phase0_only(VS, n):
    """No filter kernel runs: the similar refine over rows [0, n) and the fold alone."""
    st = _store(VS, synth_rows(9100 + n, 0, n, 384), ungrouped=min(n // 2, 40))
    _matrix(st, n)
    got = _both(st, _sources(n, 9), 200, "self")
    assert (got[2] == min(n - 1, 200)).all()
    assert st.debug_counters() == (0, 0)  # similar calls do not move the ordinary searches' counters
    st.close()


@pytest.mark.parametrize("n", [3073, 3200])
def test_first_rows_behind_phase0(VS, n):
    """kFilterPhase0 = 3,072: one row, and one 128-row tile, behind it (the int8 copy's tail and its first tile)."""
    st = _store(VS, synth_rows(9200 + n, 0, n, 384))
    _matrix(st, n)
    # the last row as a source and as somebody's neighbour: a near-duplicate of row 5 in the last row
    st.close()
    rows = synth_rows(9200 + n, 0, n, 384)
    rows[n - 1] = 0.9 * rows[5] + 0.1 * rows[n - 1]
    st = _store(VS, rows)
    for mode in MODES:
        got = _both(st, [5, n - 1], 10, mode)
        assert got[1][0][0 if mode != "none" else 1] == n - 1
    st.close()


@pytest.mark.parametrize("n", [20_000, 40_003])
def test_several_phases_and_a_ragged_tail(VS, n):
    st = _store(VS, synth_rows(9300 + n % 1000, 0, n, 384))
    assert st.filter_state()[0] == 2  # the int8 copy serves
    _matrix(st, n, ks=KS + ((1000,) if n == 20_000 else ()))
    assert st.debug_counters() == (0, 0) and st.filter_state()[2] == 0
    st.close()


@pytest.mark.parametrize("dim", [768, 1024])
def test_other_dims(VS, dim):
    n = 12_000
    st = _store(VS, synth_rows(9400 + dim, 0, n, dim))
    _matrix(st, n)
    st.close()


def test_a_dim_without_filter_kernels_scans(VS):
    n = 5000
    st = _store(VS, synth_rows(9450, 0, n, 100))
    for nq, k, mode in itertools.product((1, 9), (10,), MODES):
        _both(st, _sources(n, nq), k, mode, filtered=False)  # FILTER forced, counted as a scan, same bytes
    st.close()


def test_f16_copy(VS, monkeypatch):
    """CS_FILTER_INT8=0 at cs_index_create: the filter's operand is the f16 copy, built by the first search that needs it."""
    monkeypatch.setenv("CS_FILTER_INT8", "0")
    n = 20_000
    st = _store(VS, synth_rows(9500, 0, n, 384))
    assert st.filter_state()[0] == 1
    _matrix(st, n)
    assert st.filter_state()[0] == 1
    st.close()


def test_min_cos_is_a_strict_bound_on_both_routes(VS):
    n, k = 20_000, 10
    st = _store(VS, synth_rows(9600, 0, n, 384))
    srcs = _sources(n, 9)
    for mode in MODES:
        st.set_similar_route("scan")
        cos, ids, cnt = st.similar_raw(srcs, k, exclude=mode)
        fifth = float(cos[0][4])  # the cosine the scan route returned at rank 5 (index 4) for the first source
        assert cos[0][3] > cos[0][4]
        got = _both(st, srcs, k, mode, min_cos=fifth)
        assert got[2][0] == 4 and got[1][0][:4].tobytes() == ids[0][:4].tobytes()  # strict: that row and all under it are gone
        assert fifth not in got[0][0][:4].tolist()
        for bound in (0.0, 0.1, 0.5):
            _both(st, srcs, k, mode, min_cos=bound)
        # a bound above every cosine: nothing on both routes, and no overflow — the fold's floor keeps tau at the bound
        before = st.similar_route_info()
        got = _both(st, srcs, k, mode, min_cos=2.0)
        assert (got[2] == 0).all() and (got[1] == 0xFFFFFFFF).all() and (got[0] == 0).all()
        assert st.similar_route_info()[2] == before[2] == 0
        # ... also where the bound leaves fewer than k rows but some (a list that never fills)
        got = _both(st, srcs, 200, mode, min_cos=0.15)
        assert 0 < int(got[2].max()) < 200
    assert st.similar_route_info()[2] == 0
    st.close()


def test_ties_go_to_the_lower_id(VS):
    n, k = 20_000, 10
    rows = synth_rows(9700, 0, n, 384)
    rows[5] = rows[7000]    # a twin with a lower id inside phase 0, the source behind it
    rows[15000] = rows[40]  # a twin with a higher id behind phase 0, the source inside it
    st = _store(VS, rows)
    srcs = [7000, 5, 40, 15000, 123]
    none = _both(st, srcs, k, "none")
    assert none[1][0][:2].tolist() == [5, 7000] and none[1][1][:2].tolist() == [5, 7000]
    assert none[1][2][:2].tolist() == [40, 15000] and none[1][3][:2].tolist() == [40, 15000]
    assert none[0][0][0].tobytes() == none[0][0][1].tobytes()
    self_ = _both(st, srcs, k, "self")
    assert self_[1][:4, 0].tolist() == [5, 7000, 15000, 40]  # SELF returns the twin
    _both(st, srcs, k, "file")
    st.close()


def test_life_cycle_tombstones_and_a_reclaiming_build(VS):
    n, base, k = 20_000, 7000, 10
    rows = synth_rows(9800, 0, n, 384)
    st = _store(VS, rows, id_base=base)
    srcs = [base + r for r in (16, 17, 5000, 5001, 12_345, n - 1, 16, 3071, 3072)]
    for mode in MODES:
        _both(st, srcs, k, mode)
    # tombstones inside phase 0 and behind it, among them the first source's nearest neighbours; no reclaim yet
    st.set_similar_route("scan")
    near = [int(i) for i in st.similar_raw(srcs[:1], 6, exclude="self")[1][0]]
    first = sorted((set(near) | {base + r for r in range(3, n, 23)}) - set(srcs))
    assert len(first) * 10 < n and any(i < base + 3072 for i in first) and any(i >= base + 3072 for i in first)
    assert st.delete_chunks(first) == len(first)
    st.build_index()
    assert st.stored_rows() == n and len(st) == n - len(first)
    for mode in MODES:
        for kk in (k, 200):
            got = _both(st, srcs, kk, mode)
            assert not set(got[1].ravel().tolist()) & set(first)
    # 30 % deleted in all: the build reclaims, every surviving row behind the first hole moves, ids and groups stay
    pool = [base + r for r in range(n) if base + r not in set(srcs) and base + r not in set(first)]
    more = sorted(pool, key=lambda i: ((i - base) % 10 not in (0, 4, 8), i))[:(3 * n) // 10 - len(first)]
    assert st.delete_chunks(more) == len(more)
    st.build_index()
    gone = set(first) | set(more)
    assert st.stored_rows() == len(st) == n - len(gone)
    for mode in MODES:
        for kk in (k, 200):
            got = _both(st, srcs, kk, mode)  # sources the build moved
            assert not set(got[1].ravel().tolist()) & gone
    got = _both(st, srcs, k, "file", min_cos=0.1)
    assert st.similar_route_info()[2] == 0
    st.close()


def _hog_store(VS, rows, hog, file_of_8=False):
    n = len(rows)
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    if not file_of_8:
        groups[hog] = 0
    groups[n - 40:] = NO_GROUP
    st = VS(None, rows.shape[1])
    st.insert_embeddings(rows)
    st.build_index()
    st.set_groups(np.arange(n), groups)
    return st, groups


def test_an_excluded_hog_overflows_and_the_scan_answers(VS, oracle):
    """Rows 8,000-13,999 are near-duplicates (cosine >= 0.95) of row 8,000 and form one group; the source is row 8,000, the
    mode "file", k = 10.  All 6,000 beat the k-th best of the other rows, 6,000 > batched_cap(10) = 4,096 candidates in the
    one phase behind phase 0: the buffer overflows and the similar scan answers.  The int8 copy is not struck for it.

    "A file of 8 instead": the source's file, its near-duplicates, holds 8 rows (8,000-8,007) instead of 6,000 — excluding
    it leaves the filter nothing to overflow with.  (Regrouping the same 6,000 near-duplicates into files of 8 is another
    matter: 5,992 rows the query MAY return then beat phase 0's threshold in one phase, and the buffer overflows as the
    ordinary search's does for such a row; that case is asserted too, as a fallback with the same bytes.)"""
    n, dim, k, src = 20_000, 384, 10, 8000
    noise = synth_rows(9900, 0, n, dim)
    rows = noise.copy()
    hog = np.arange(8000, 14_000)
    rows[hog[1:]] = 0.95 * rows[src] + 0.05 * noise[hog[1:]]
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    assert float((unit[hog] @ unit[src]).min()) >= 0.95
    st, groups = _hog_store(VS, rows, hog)
    assert st.filter_state()[0] == 2
    queries = synth_rows(9901, 0, 4, dim)
    state0, counters0 = st.filter_state(), st.debug_counters()
    for rep in range(3):
        state, counters = st.filter_state(), st.debug_counters()
        got = _both(st, [src], k, "file", fallbacks=1)  # filter_fallbacks moves by exactly 1
        assert st.filter_state() == state and st.debug_counters() == counters
        if rep == 0:
            oc, oi = oracle.scan_topk(rows, rows[src], n, mode="omp")
            ec, ei = drop_excluded(oc, oi, groups[oi], src, int(groups[src]), "file", None, k)
            assert got[2][0] == k and got[1][0].tolist() == ei
            assert np.abs(got[0][0] - np.asarray(ec, np.float32)).max() < 1e-4
            assert not (groups[got[1][0]] == 0).any()
        for _ in range(2):  # ordinary searches through the same pooled workspace: none is struck for the similar call's overflow
            c, i, cnt = st.search_raw(queries, k)
            assert (cnt == k).all()
    assert st.filter_state()[0] == 2 and st.filter_state()[2] == 0  # the int8 copy still serves; no f16 rerun
    assert st.filter_state() == state0
    assert st.debug_counters() == (counters0[0] + 6, counters0[1])
    # nine sources, one of them inside the hog: the call falls back as a whole, every list exact
    _both(st, [src, 16, 17, 100, n - 1, 16, 23, 0, 7], k, "file", fallbacks=1)
    # ordinary sources alone do not (row 0 is left out: its cosine with row 8,000 is 0.128, inside the int8 band under the
    # 0.131 its phase 0 leaves as the threshold, so all 6,000 become its candidates — the ordinary search's overflow, for
    # which that search reruns on the f16 copy; here the scan answers, as asserted above)
    _both(st, [16, 17, 100, n - 1, 16, 23, 8, 7], k, "file")
    st.close()
    # the 6,000 near-duplicates regrouped into files of 8: not excluded, and still more than the buffer holds in one phase
    st, groups = _hog_store(VS, rows, hog, file_of_8=True)
    _both(st, [src], k, "file", fallbacks=1)
    st.close()
    # the source's file holds 8 near-duplicates instead of 6,000: no fallback
    rows8 = noise.copy()
    rows8[8001:8008] = 0.95 * rows8[src] + 0.05 * noise[8001:8008]
    st, groups = _hog_store(VS, rows8, hog, file_of_8=True)
    got = _both(st, [src], k, "file")
    assert not set(got[1][0].tolist()) & set(range(8000, 8008))
    got = _both(st, [src], k, "self")
    assert sorted(got[1][0][:7].tolist()) == list(range(8001, 8008))
    assert st.similar_route_info()[2] == 0
    st.close()


def test_concurrent_similar_searches_on_the_filter_route(VS):
    n, dim, k = 20_000, 384, 25
    st = _store(VS, synth_rows(9950, 0, n, dim))
    rng = np.random.default_rng(12)
    jobs = [(rng.integers(0, n, nq).tolist(), mode, bound) for nq, mode, bound in
            [(1, "self", None), (3, "file", None), (9, "none", 0.0), (40, "file", 0.05)]]
    st.set_similar_route("scan")
    want = [st.similar_raw(s, k, exclude=m, min_cos=b) for s, m, b in jobs]
    assert all(int(w[2].max()) > 0 for w in want)
    st.set_similar_route("filter")
    before = st.similar_route_info()
    errors = []

    def work(t):
        try:
            s, m, b = jobs[t]
            for _ in range(8):
                r = st.similar_raw(s, k, exclude=m, min_cos=b)
                if not all(x.tobytes() == y.tobytes() for x, y in zip(r, want[t])):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    after = st.similar_route_info()
    assert after == (before[0] + 32, before[1], before[2])
    st.close()


def test_interface(VS, gpu_lib, monkeypatch):
    n, k = 20_000, 10
    st = _store(VS, synth_rows(9960, 0, n, 384))
    assert st.similar_route_info() == (0, 0, 0)
    for bad in (-1, 3, 7):
        assert gpu_lib.cs_index_set_similar_route(st.handle, bad) == _lib.CS_ERR_BAD_ARG
        assert "route must be CS_SIMILAR_ROUTE_AUTO, _SCAN or _FILTER" in _lib.last_error()
    assert gpu_lib.cs_index_set_similar_route(None, 0) == _lib.CS_ERR_BAD_ARG and "null index handle" in _lib.last_error()
    assert gpu_lib.cs_index_similar_route_info(None, None, None, None) == _lib.CS_ERR_BAD_ARG
    assert gpu_lib.cs_index_similar_route_info(st.handle, None, None, None) == _lib.CS_OK
    with pytest.raises(_lib.CsError):
        st.set_similar_route(5)
    # AUTO (the default) follows the ordinary search's route: nine sources filter, two over 10,000..16,383 rows would scan,
    # one source over fewer than 32,768 rows scans
    srcs = _sources(n, 9)
    st.similar_raw(srcs, k)
    assert st.similar_route_info() == (1, 0, 0)
    st.similar_raw(srcs[:1], k)
    assert st.similar_route_info() == (1, 1, 0)
    _both(st, srcs, k, "file", route="auto")
    _both(st, srcs[:1], k, "file", route="auto", filtered=False)
    # the scoped call keeps to its gathered scan and does not move the counters, whatever the route
    sc = st.scope(np.arange(0, n, 3))
    for route in ("auto", "scan", "filter"):
        st.set_similar_route(route)
        before = st.similar_route_info()
        a = st.similar_raw(srcs, k, exclude="file", scope=sc)
        assert st.similar_route_info() == before
        if route != "auto":
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, first))
        first = a
    sc.close()
    st.close()
    # CS_SIMILAR_ROUTE at cs_index_create
    monkeypatch.setenv("CS_SIMILAR_ROUTE", "scan")
    st = _store(VS, synth_rows(9960, 0, n, 384))
    st.similar_raw(srcs, k)
    assert st.similar_route_info() == (0, 1, 0)
    st.close()
    monkeypatch.setenv("CS_SIMILAR_ROUTE", "filter")
    st = _store(VS, synth_rows(9960, 0, n, 384))
    st.similar_raw(srcs[:1], k)
    assert st.similar_route_info() == (1, 0, 0)
    st.close()
