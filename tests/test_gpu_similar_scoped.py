"""Similar-chunk search inside a scope (cs_index_search_similar_scoped, codesearch_amd/csrc/scan_similar.hip part 4): the
exact best k chunks OF A SCOPE for a query that is a stored chunk — in the scope or not — without the chunk, or without
the chunk's whole file, decided inside the selection.

Ground truth comes only from code that exists without the feature: the source's row read back (read_rows), the full
(cosine desc, id asc) order of the scope for it — search_raw(row, live scope rows, scope=) on the gathered route, one call
for a scope of at most 1,024 ids, with its cosine bits — reduced on the host by search.drop_excluded.  Ids, counts and
cosine bytes must be equal; unused slots hold 0xFFFFFFFF / 0."""
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, drop_excluded
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

MODES = ("none", "self", "file")
SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1000, 1), (10, 40)]  # (k, nq): query tiles 1, 2, 4, a ragged last tile, deep


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows, id_base=0):
    st = VS(None, rows.shape[1], id_base=id_base)
    st.insert_embeddings(rows)
    st.build_index()
    return st


def _scope(st, ids):
    sc = st.scope(ids)
    assert len(sc) <= 1024  # one scoped search returns the whole order
    sc.set_route("gather")
    return sc


def _scope_order(st, sc, q):
    """(cos, ids) of every live row of the scope, (cosine desc, id asc): one scoped search on the gathered route at
    k = the scope's ids; its count is the number of live rows."""
    if len(sc) == 0:
        return np.zeros(0, np.float32), np.zeros(0, np.uint32)
    c, i, cnt = st.search_raw(q, len(sc), scope=sc)
    return c[0][:cnt[0]].copy(), i[0][:cnt[0]].copy()


def _truth(st, sc, srcs):
    """{source id: the scope's full order for that source's stored row}, one scoped search per distinct source."""
    return {s: _scope_order(st, sc, st.read_rows(s - st.id_base, 1)[0]) for s in sorted(set(int(x) for x in srcs))}


def _files_of_8(n, ungrouped, base=0):
    """ids in files of 8 consecutive ids; the last `ungrouped` ids carry no group."""
    return {base + r: r // 8 for r in range(n - ungrouped)}


def _group_lookup(groups: dict):
    return lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]


def _check(st, sc, truth, lookup, srcs, k, mode, min_cos=None):
    """st.similar_raw(srcs, k, mode, min_cos, scope=sc) against truth[source] reduced on the host; -> the counts."""
    cos, ids, cnt = st.similar_raw(srcs, k, exclude=mode, min_cos=min_cos, scope=sc)
    assert cos.shape == ids.shape == (len(srcs), k) and cnt.shape == (len(srcs),)
    for q, s in enumerate(int(x) for x in srcs):
        tc, ti = truth[s]
        ec, ei = drop_excluded(tc, ti, lookup(ti), s, lookup([s])[0], mode, min_cos, k)
        n = len(ei)
        assert cnt[q] == n, (q, s, k, mode, cnt[q], n)
        assert ids[q][:n].tolist() == ei, (q, s, k, mode)
        assert cos[q][:n].tobytes() == np.asarray(ec, np.float32).tobytes(), (q, s, k, mode)
        assert (ids[q][n:] == 0xFFFFFFFF).all() and (cos[q][n:] == 0).all()
    return cnt


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# one query tile of four holds two sources of one file (16, 17), one of another (100) and an ungrouped one (970); 16, 970 and
# 100 come twice; 300 and 301 lie in the contiguous and the ragged scope, 17 / 23 / 959 / 999 are odd
SOURCES = [16, 17, 100, 970, 16, 23, 999, 300, 301, 8, 960, 959, 500, 501, 502, 503, 970, 100]


def _scope_ids(n):
    return {
        "all": np.arange(n),
        "even": np.arange(0, n, 2),                  # each file half in the scope
        "contiguous": np.arange(200, 456),
        "one": [100],
        "seven": [3, 16, 17, 100, 501, 970, 999],    # shorter than one tile of any U
        "ragged": np.arange(284, 317),               # 33 ids: a ragged last tile
    }


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_similar_scoped_equals_reduced_scoped_order(VS, dim):
    n, seed = 1000, 9600 + dim
    st = _store(VS, synth_rows(seed, 0, n, dim))
    srcs = SOURCES + [int(x) for x in np.random.default_rng(seed).integers(0, n, 40 - len(SOURCES))]
    scopes = {name: _scope(st, ids) for name, ids in _scope_ids(n).items()}
    truths = {name: _truth(st, sc, srcs) for name, sc in scopes.items()}
    for name, ids in _scope_ids(n).items():  # sources inside and outside each scope, within the first nine
        inside = set(int(i) for i in ids)
        assert any(s in inside for s in srcs[:9]) and (name == "all" or any(s not in inside for s in srcs[:9]))
    # no group assigned: "file" is "self"
    for k, nq in SHAPES:
        assert _same(st.similar_raw(srcs[:nq], k, exclude="file", scope=scopes["even"]),
                     st.similar_raw(srcs[:nq], k, exclude="self", scope=scopes["even"]))
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    for name, sc in scopes.items():
        for mode in MODES:
            for k, nq in SHAPES:
                cnt = _check(st, sc, truths[name], look, srcs[:nq], k, mode)
                if k == 1000 and name == "even":  # 500 rows, 4 of each file; the source 16 is in the scope and grouped
                    assert cnt[0] == {"none": 500, "self": 499, "file": 496}[mode]
    for mode in MODES:  # an odd grouped source: not in the scope itself, four rows of its file are
        cnt = _check(st, scopes["even"], truths["even"], look, [17], 1000, mode)
        assert cnt[0] == {"none": 500, "self": 500, "file": 496}[mode]
        # EXCLUDE_SELF with a source outside the scope is EXCLUDE_NONE
    assert _same(st.similar_raw([17, 23], 200, exclude="self", scope=scopes["even"]),
                 st.similar_raw([17, 23], 200, exclude="none", scope=scopes["even"]))
    st.close()


@pytest.mark.parametrize("dim", [384, 100])
def test_identities(VS, dim):
    n = 1000
    rows = synth_rows(9650 + dim, 0, n, dim)
    rows[5] = rows[700]  # an identical row with a lower id: it wins the tie
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    every = _scope(st, np.arange(n))
    part = _scope(st, [5, 700] + list(range(1, n, 3)))
    srcs = [700, 5] + SOURCES + [int(x) for x in np.random.default_rng(dim).integers(0, n, 20)]
    # a scope that holds every issued id: the unscoped similar search, byte for byte
    for mode in MODES:
        for k, nq in SHAPES:
            for bound in (None, 0.02):
                assert _same(st.similar_raw(srcs[:nq], k, exclude=mode, min_cos=bound, scope=every),
                             st.similar_raw(srcs[:nq], k, exclude=mode, min_cos=bound)), (mode, k, nq, bound)
    # EXCLUDE_NONE without a bound: the scoped search (gathered route) of the row read back
    for k in (1, 10, 200):
        cos, ids, cnt = st.similar_raw(srcs[:9], k, exclude="none", scope=part)
        for q, s in enumerate(srcs[:9]):
            want = st.search_raw(st.read_rows(s, 1)[0], k, scope=part)
            assert cnt[q] == want[2][0] == k
            assert ids[q].tobytes() == want[1][0].tobytes() and cos[q].tobytes() == want[0][0].tobytes()
    # the tie: the lower id first, with the same cosine bits; excluding the source leaves its twin first
    cos, ids, cnt = st.similar_raw([700, 5], 10, exclude="none", scope=part)
    assert ids[0][:2].tolist() == [5, 700] and ids[1][:2].tolist() == [5, 700]
    assert cos[0][0].tobytes() == cos[0][1].tobytes()
    cos, ids, cnt = st.similar_raw([700, 5], 10, exclude="self", scope=part)
    assert ids[0][0] == 5 and ids[1][0] == 700
    # a source's own answer does not depend on its neighbours in the call
    alone = st.similar_raw([970], 10, exclude="file", scope=part)
    batch = st.similar_raw(srcs[:9], 10, exclude="file", scope=part)
    assert srcs[5] == 970 and all(x[0].tobytes() == y[5].tobytes() for x, y in zip(alone, batch))
    st.close()


def test_min_cos_is_a_strict_bound(VS):
    n, dim = 1000, 384
    st = _store(VS, synth_rows(9801, 0, n, dim))
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    sc = _scope(st, np.arange(0, n, 2))
    srcs = [50, 51, 975]
    truth = _truth(st, sc, srcs)
    for mode in MODES:
        kept_c, _ = drop_excluded(*truth[50], look(truth[50][1]), 50, groups[50], mode, None, 20)
        fourth, fifth = np.float32(kept_c[3]), np.float32(kept_c[4])
        assert fourth > fifth  # distinct cosines
        between = np.float32((np.float64(fourth) + np.float64(fifth)) / 2)
        assert fourth > between > fifth
        assert _check(st, sc, truth, look, [50], 20, mode, min_cos=between)[0] == 4
        assert _check(st, sc, truth, look, [50], 20, mode, min_cos=fifth)[0] == 4  # strict: the 5th is not above itself
        for k, m in [(10, float(fifth)), (200, 0.0), (1000, -0.02), (10, 0.05)]:
            _check(st, sc, truth, look, srcs, k, mode, min_cos=np.float32(m))
        cos, ids, cnt = st.similar_raw(srcs, 10, exclude=mode, min_cos=2.0, scope=sc)  # above every cosine
        assert (cnt == 0).all() and (ids == 0xFFFFFFFF).all() and (cos == 0).all()
        assert _same(st.similar_raw(srcs, 10, exclude=mode, min_cos=float("-inf"), scope=sc),
                     st.similar_raw(srcs, 10, exclude=mode, scope=sc))
    st.close()


def test_a_hog_file_inside_the_scope_does_not_crowd_out_the_rest(VS):
    """600 rows of the source's file are 0.95 s + 0.05 noise; the scope is that file and 100 other rows.  Excluding the file
    inside the selection returns ten of the other rows; what a caller can do without it — the scoped search of the row at
    k + 1, the file dropped from the ranked list — returns none of them."""
    n, dim, k = 1000, 384, 10
    rows = synth_rows(9701, 0, n, dim)
    hog = np.arange(200, 800)
    src = 200
    rows[hog[1:]] = 0.95 * rows[src] + 0.05 * rows[hog[1:]]
    groups = {r: 1000 + r // 8 for r in range(n)}
    groups.update({int(r): 7 for r in hog})
    st = _store(VS, rows)
    st.set_groups(list(groups), list(groups.values()))
    others = list(range(0, 100, 2)) + list(range(900, 1000, 2))
    sc = _scope(st, list(hog) + others)
    truth = _truth(st, sc, [src, 201, 0, 1])
    look = _group_lookup(groups)
    assert _check(st, sc, truth, look, [src], k, "file")[0] == k
    got = st.similar_raw([src], k, exclude="file", scope=sc)[1][0].tolist()
    assert set(got) <= set(others)
    c, i, c_n = st.search_raw(st.read_rows(src, 1)[0], k + 1, scope=sc)
    assert [x for x in i[0][:c_n[0]].tolist() if groups[x] != 7] == []  # the rank-then-filter a caller is left with today
    _check(st, sc, truth, look, [src, 201, 0, 1], k, "self")
    cnt = _check(st, sc, truth, look, [src, 201, 0, 1], 200, "file")
    assert cnt.tolist() == [100, 100, 200, 200]
    st.close()


def test_similar_scoped_follows_the_store_life_cycle(VS):
    n, dim, base, k = 900, 384, 5000, 10
    rows = synth_rows(9911, 0, n, dim)
    st = _store(VS, rows, id_base=base)
    groups = _files_of_8(n, 0, base)
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    src = base + 101
    srcs = [src, base + 102, base + 899, base]
    later = [base + n + j for j in range(6)]  # not issued yet: they match once they are
    sc = _scope(st, [base + r for r in range(0, n, 2)] + later)
    small = _scope(st, [base + r for r in range(600, 640, 2)])
    assert sc.info()[1] == n // 2

    def check_all(t):
        for mode in MODES:
            for kk in (k, 200):
                _check(st, sc, t, look, srcs, kk, mode)

    truth = _truth(st, sc, srcs)
    check_all(truth)
    # a third of the rows go: the source's nearest neighbours in the scope, every row of `small`, part of the scope
    near = [int(i) for i in truth[src][1][:5] if int(i) not in srcs]
    pool = [base + r for r in range(n) if base + r not in srcs]
    gone = sorted(set(near) | set(int(i) for i in small.ids) | set(i for i in pool if (i - base) % 10 in (0, 3, 7)))
    gone = gone + [i for i in pool if i not in set(gone)][:n // 3 - len(gone)]
    assert len(gone) == n // 3 and st.delete_chunks(gone) == len(gone)
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.similar_raw(srcs, k, scope=sc)
    st.build_index()
    assert st.stored_rows() == len(st) == n - len(gone)  # the build reclaimed: rows moved, ids and groups stay
    truth = _truth(st, sc, srcs)
    alive_in_scope = [int(i) for i in sc.ids if int(i) not in set(gone) and int(i) < base + n]
    assert sorted(truth[src][1].tolist()) == alive_in_scope and 0 < len(alive_in_scope) < n // 2
    check_all(truth)
    assert not set(st.similar_raw([src], k, exclude="self", scope=sc)[1][0].tolist()) & set(near)
    # every row of the scope deleted: counts 0, no error
    cos, ids, cnt = st.similar_raw(srcs, k, exclude="self", scope=small)
    assert (cnt == 0).all() and (ids == 0xFFFFFFFF).all() and (cos == 0).all() and small.info()[1] == 0
    with pytest.raises(_lib.CsError, match=r"ids\[1\] = %d: the chunk was deleted" % gone[0]):
        st.similar_raw([src, gone[0]], k, scope=sc)
    # appended rows whose ids the scope already holds are found once they are issued
    s_row = st.read_rows(src - base, 1)[0]
    new = st.insert_embeddings(np.stack([0.95 * s_row + 0.05 * rows[j] for j in range(6)])).tolist()
    assert new == later
    st.build_index()
    truth = _truth(st, sc, srcs + new[:1])
    check_all(truth)
    for mode in ("self", "file"):  # (the new rows carry no group: "file" keeps them)
        assert sorted(st.similar_raw([src], 6, exclude=mode, scope=sc)[1][0].tolist()) == new
    _check(st, sc, truth, look, [new[0], src], k, "file")
    # emptied, then refilled: the answers come under the ids issued since
    everything = [base + r for r in range(n) if base + r not in set(gone)] + new
    assert st.delete_chunks(everything) == len(everything)
    st.build_index()
    assert len(st) == 0
    with pytest.raises(_lib.CsError, match="the chunk was deleted"):
        st.similar_raw([src], k, scope=sc)
    again = st.insert_embeddings(synth_rows(9912, 0, 300, dim)).tolist()
    assert again[0] == base + n + 6
    st.build_index()
    groups2 = {i: j // 8 for j, i in enumerate(again)}
    st.set_groups(list(groups2), list(groups2.values()))
    sc2 = _scope(st, again[::2])
    srcs2 = [again[0], again[1], again[299]]
    t2 = _truth(st, sc2, srcs2)
    for mode in MODES:
        cnt = _check(st, sc2, t2, _group_lookup(groups2), srcs2, 200, mode)
        assert cnt.tolist() == {"none": [150] * 3, "self": [149, 150, 150], "file": [146, 146, 148]}[mode]
    cos, ids, cnt = st.similar_raw(srcs2, k, scope=sc)  # the old scope holds none of the new ids
    assert (cnt == 0).all()
    st.close()


def _raw_call(lib, h, scope, ids, nq, k, exclude, min_cos, cos, out_ids, counts):
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    return lib.cs_index_search_similar_scoped(h, scope, p(ids, _lib.u32p), nq, k, exclude, min_cos, p(cos, _lib.f32p),
                                              p(out_ids, _lib.u32p), p(counts, _lib.u32p))


def test_errors_and_their_order(VS, gpu_lib):
    n, dim, k = 500, 384, 5
    st = VS(None, dim, id_base=100)
    st.insert_embeddings(synth_rows(9931, 0, n, dim))
    other = _store(VS, synth_rows(9932, 0, 50, dim))
    foreign = other.scope(np.arange(50))
    sc = st.scope(np.arange(100, 400))  # made on a store not built: the first search makes the list
    empty = st.scope([])
    src = np.array([100, 101], np.uint32)
    cos = np.full((2, k), 7.0, np.float32)
    ids = np.full((2, k), 7, np.uint32)
    counts = np.full(2, 7, np.uint32)
    nan, inf = float("nan"), float("-inf")

    def state():
        return [s.info()[2] for s in (sc, empty, foreign)] + [s.route_info()[1] for s in (sc, empty, foreign)]

    def fails(text, scope, *a, handle=True, status=_lib.CS_ERR_BAD_ARG):
        before = state()
        assert _raw_call(gpu_lib, st.handle if handle else None, scope and scope.handle, *a) == status
        assert text in _lib.last_error(), _lib.last_error()
        assert (cos == 7.0).all() and (ids == 7).all() and (counts == 7).all()  # a failing call writes nothing,
        assert state() == before                                               # refreshes no list and counts no search

    # 1. cs_index_search_similar's own, in its order, each before everything behind it (a null scope included)
    fails("null index handle", None, None, 0, 0, 9, nan, None, None, None, handle=False)
    fails("Index not built. Call build_index() after inserting chunks.", None, None, 0, 0, 9, nan, None, None, None,
          status=_lib.CS_ERR_NOT_BUILT)
    st.build_index()
    assert sc.info()[2] == 0  # the list is still to be made: a failing call must not make it
    fails("nq must be in 1..4096, got 0", None, None, 0, 0, 9, nan, None, None, None)
    fails("nq must be in 1..4096, got 4097", None, None, 4097, 0, 9, nan, None, None, None)
    fails("k must be in 1..1024, got 0", None, None, 2, 0, 9, nan, None, None, None)
    fails("k must be in 1..1024, got 1025", None, None, 2, 1025, 9, nan, None, None, None)
    fails("null buffer", None, None, 2, k, 9, nan, cos, ids, counts)
    fails("null buffer", None, src, 2, k, 9, nan, None, ids, counts)
    fails("null buffer", None, src, 2, k, 9, nan, cos, None, counts)
    fails("null buffer", None, src, 2, k, 9, nan, cos, ids, None)
    bad = np.array([100, 99], np.uint32)
    fails("exclude must be", None, bad, 2, k, 3, nan, cos, ids, counts)
    fails("exclude must be", foreign, bad, 2, k, -1, nan, cos, ids, counts)
    fails("min_cos is NaN", sc, src, 2, k, 2, nan, cos, ids, counts)
    fails("min_cos is NaN", foreign, bad, 2, k, 2, nan, cos, ids, counts)  # NaN bound + foreign scope -> NaN
    fails("min_cos is NaN", None, bad, 2, k, 2, nan, cos, ids, counts)
    # 2. the scope: null, then made for another store — before the ids
    fails("null scope handle", None, src, 2, k, 1, inf, cos, ids, counts)
    fails("null scope handle", None, bad, 2, k, 1, inf, cos, ids, counts)
    fails("the scope was made for another store", foreign, src, 2, k, 1, inf, cos, ids, counts)
    assert st.delete_chunks([150]) == 1
    st.build_index()
    gone = np.array([100, 150, 99], np.uint32)
    fails("the scope was made for another store", foreign, gone, 3, k, 1, inf, cos, ids, counts)  # + deleted id -> scope
    # 3. the ids: the first offending one is named; an empty scope does not turn the id error into an empty answer
    fails("ids[1] = 99 was never issued", sc, bad, 2, k, 2, inf, cos, ids, counts)
    fails("ids[0] = 600 was never issued", sc, np.array([600, 99], np.uint32), 2, k, 0, 0.5, cos, ids, counts)
    fails("ids[1] = 150: the chunk was deleted", sc, gone, 3, k, 1, inf, cos, ids, counts)
    fails("ids[0] = 99 was never issued", sc, np.array([99, 150], np.uint32), 2, k, 1, inf, cos, ids, counts)
    fails("ids[1] = 99 was never issued", empty, bad, 2, k, 1, inf, cos, ids, counts)
    fails("ids[0] = 150: the chunk was deleted", empty, np.array([150], np.uint32), 1, k, 1, inf, cos, ids, counts)
    assert sc.info()[2] == 0 and sc.route_info()[1] == 0
    # success: the list is made once, every library call counts as one gathered search whatever the scope's route
    sc.set_route("filter")
    assert _raw_call(gpu_lib, st.handle, sc.handle, src, 2, k, 1, inf, cos, ids, counts) == _lib.CS_OK
    assert counts.tolist() == [k, k] and (ids != 7).all() and sc.info()[2] == 1 and sc.route_info()[:2] == (0, 1)
    assert _raw_call(gpu_lib, st.handle, empty.handle, src, 2, k, 1, inf, cos, ids, counts) == _lib.CS_OK
    assert counts.tolist() == [0, 0] and (ids == 0xFFFFFFFF).all() and (cos == 0).all()
    many = np.arange(4100) % 50 + 100
    got = st.similar_raw(many, 1, scope=sc)  # 4,100 sources: two library calls
    assert sc.route_info()[:2] == (0, 3) and sc.info()[2] == 1
    once = st.similar_raw(np.arange(100, 150), 1, scope=sc)
    assert got[1].tobytes() == once[1][many - 100].tobytes() and got[0].tobytes() == once[0][many - 100].tobytes()
    assert (got[2] == 1).all() and (got[1][:, 0] != many).all()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="exclude must be"):
        st.similar_raw([100], k, exclude="group", scope=sc)
    with pytest.raises(_lib.CsError, match="nq must be in 1..4096, got 0"):
        st.similar_raw([], k, scope=sc)
    with pytest.raises(_lib.CsError, match="the scope was made for another store"):
        st.similar_raw([100], k, scope=foreign)
    done = st.scope([100, 101])
    done.close()
    for call in (lambda: st.similar_raw([100], k, scope=done), lambda: st.similar(100, k, scope=done)):
        with pytest.raises(_lib.CsError, match="scope is closed") as e:
            call()
        assert e.value.code == _lib.CS_ERR_BAD_ARG
    other.close()
    st.close()


def test_a_sharded_store_and_its_scopes_are_refused(VS, gpu_lib):
    dim, k = 384, 5
    st = _store(VS, synth_rows(9933, 0, 64, dim))
    sharded = VS(None, dim, devices=[0, 0])
    sharded.insert_embeddings(synth_rows(9934, 0, 64, dim))
    sharded.build_index()
    over_shards = sharded.scope(np.arange(64))
    for call in (lambda: sharded.similar_raw([0], k, scope=over_shards), lambda: sharded.similar(0, k, scope=over_shards)):
        with pytest.raises(_lib.CsError, match="no similar-chunk search: no cs_shards_ form yet") as e:
            call()
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    with pytest.raises(_lib.CsError, match="the scope was made for another store") as e:  # as the other single-index calls
        st.similar_raw([0], k, scope=over_shards)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    sharded.close()
    st.close()


def test_concurrent_similar_scoped_searches(VS):
    n, dim, k = 3000, 384, 25
    st = _store(VS, synth_rows(9941, 0, n, dim))
    st.set_groups(np.arange(n), np.arange(n) // 8)
    rng = np.random.default_rng(11)
    a, b = st.scope(np.arange(0, n, 2)), st.scope(rng.choice(n, 700, replace=False))
    jobs = [(rng.integers(0, n, nq).tolist(), mode, bound, sc) for nq, mode, bound, sc in
            [(1, "self", None, a), (3, "file", None, b), (9, "none", 0.0, a), (2, "file", 0.05, b)]]
    want = [st.similar_raw(s, k, exclude=m, min_cos=bd, scope=sc) for s, m, bd, sc in jobs]
    assert all(int(w[2].max()) > 0 for w in want)
    before = [sc.route_info()[1] for sc in (a, b)]
    errors = []

    def work(t):
        try:
            s, m, bd, sc = jobs[t]
            for _ in range(20):
                if not _same(st.similar_raw(s, k, exclude=m, min_cos=bd, scope=sc), want[t]):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(jobs))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    assert [sc.route_info()[1] for sc in (a, b)] == [before[0] + 40, before[1] + 40]
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_similar_with_a_scope_returns_results_with_metadata(VS):
    dim, per = 384, 12
    files = ["vendor/gen.rs", "src/a.rs", "src/b.rs", "tests/c.rs", "lib/d.rs"]
    noise = synth_rows(9951, 0, per * len(files), dim)
    paths = [files[i % len(files)] for i in range(len(noise))]
    rows = noise.copy()
    hog = [i for i, p in enumerate(paths) if p == files[0]]
    src = hog[0]
    rows[hog[1:]] = 0.9 * rows[src] + 0.1 * noise[hog[1:]]  # vendor/gen.rs: near-duplicates of its first chunk
    st = VS(None, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(len(paths)))
    st.build_index()
    under_src = st.chunk_ids_under("src/")
    assert len(under_src) == 2 * per
    sc = _scope(st, under_src)
    full_c, full_i = _scope_order(st, sc, st.read_rows(src, 1)[0])
    got = st.similar(src, 5, scope=sc)  # "where else under src/ is this copied": the source is in vendor/
    assert [r.id for r in got] == full_i[:5].tolist() and {r.path for r in got} <= {"src/a.rs", "src/b.rs"}
    assert [r.content for r in got] == [f"chunk {i}" for i in full_i[:5]]
    assert [r.id for r in st.similar(src, 5, other_files=True, scope=sc)] == [r.id for r in got]
    inside = under_src[0]
    full_c, full_i = _scope_order(st, sc, st.read_rows(inside, 1)[0])
    number = {}
    look = [number.setdefault(paths[int(i)], len(number)) for i in full_i]
    want = drop_excluded(full_c, full_i, look, inside, number[paths[inside]], "file", None, 5)[1]
    other = st.similar(inside, 5, other_files=True, scope=sc)
    assert [r.id for r in other] == want and paths[inside] not in {r.path for r in other}
    assert st.similar(inside, 5, min_score=1.0, scope=sc) == []
    st.close()


def test_cpp_wrapper_finds_similar_chunks_inside_a_scope():
    """host/codesearch_gpu.hpp: VectorStore::similar(id, limit, other_files, scope) (tests/cpp/similar_scoped_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "similar_scoped_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "similar_scoped_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "similar scoped host ok" in r.stdout
