"""Scope algebra on the device (cs_scope_combine, cs_*_scope_create_range, cs_scope_read_ids; codesearch_amd/csrc/
scope_ops.hip): union, intersection and difference of two scopes, and range scopes.

THE RULE under test: the combined scope answers every scoped call bit for bit as its TWIN does — a scope made by
VectorStore.scope() from numpy's set operation on the two id arrays (np.union1d / intersect1d / setdiff1d), code that exists
without the feature.  The id sets themselves are compared byte for byte through cs_scope_read_ids.  Tiles: T =
cs_scope_ops_tile() ids of a + b per block; the lengths and the planted runs below are built from T, so a duplicate falls on
the last position of one tile and the first of the next."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

NUMPY_OPS = {"union": np.union1d, "intersection": np.intersect1d, "difference": np.setdiff1d}


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


@pytest.fixture(scope="module")
def small(VS):
    """A built 1,000-row store: the id sets of the set tests need not be issued ids."""
    st = VS(None, 384)
    st.insert_embeddings(synth_rows(4101, 0, 1000, 384))
    st.build_index()
    yield st
    st.close()


def _u32(x):
    return np.ascontiguousarray(x, np.uint32)


def _host_op(op, a, b):
    return _u32(NUMPY_OPS[op](_u32(a), _u32(b)))


def _check_sets(st, a_ids, b_ids):
    """a op b and b op a for the three ops: read_ids equals numpy's answer byte for byte, and so does the length."""
    a_ids, b_ids = _u32(a_ids), _u32(b_ids)
    with st.scope(a_ids) as a, st.scope(b_ids) as b:
        assert a.ids.tobytes() == a_ids.tobytes() and b.ids.tobytes() == b_ids.tobytes()  # (the inputs were ascending)
        for x, y, xi, yi in ((a, b, a_ids, b_ids), (b, a, b_ids, a_ids)):
            for op in ("union", "intersection", "difference"):
                want = _host_op(op, xi, yi)
                with getattr(x, op)(y) as got:
                    assert len(got) == want.size == got.info()[0], (op, len(got), want.size)
                    ids = got.ids
                    assert ids.dtype == np.uint32 and ids.tobytes() == want.tobytes(), \
                        (op, xi.size, yi.size, np.flatnonzero(ids[:min(ids.size, want.size)] != want[:min(ids.size, want.size)])[:4])
                    assert got.ids is ids  # read back once, then kept


def _random_set(rng, n, hi):
    return np.sort(rng.choice(hi, n, replace=False)).astype(np.uint32)


# ---- 1. sets alone ---------------------------------------------------------------------------------------------------

def test_tile_is_what_the_plan_header_says(gpu_lib):
    t = int(gpu_lib.cs_scope_ops_tile())
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    plan = open(os.path.join(root, "codesearch_amd", "csrc", "scope_ops_plan.hpp")).read()
    assert t >= 256 and t % 256 == 0 and "kScopeOpsTile" in plan


def test_sets_of_every_length_around_a_tile(small, gpu_lib):
    T = int(gpu_lib.cs_scope_ops_tile())
    rng = np.random.default_rng(11)
    lens = [0, 1, T - 1, T, T + 1, 3 * T + 1]
    for la in lens:
        for lb in lens:
            _check_sets(small, _random_set(rng, la, 4 * T + 16), _random_set(rng, lb, 4 * T + 16))


def test_identical_disjoint_and_alternating_sets(small, gpu_lib):
    T = int(gpu_lib.cs_scope_ops_tile())
    rng = np.random.default_rng(12)
    s = _random_set(rng, 2 * T + 7, 1 << 20)
    _check_sets(small, s, s.copy())                                         # identical (two handles)
    _check_sets(small, np.arange(0, 3 * T, 2), np.arange(1, 3 * T, 2))      # every second id: disjoint, interleaved
    _check_sets(small, np.arange(5, 5 + 2 * T), np.arange(5 + 2 * T, 5 + 3 * T + 3))  # disjoint, one behind the other
    _check_sets(small, s, s[::3])                                           # one inside the other
    with small.scope(s) as a:                                               # a == b: the same handle twice
        with a | a as u, a & a as i, a - a as d:
            assert u.ids.tobytes() == s.tobytes() and i.ids.tobytes() == s.tobytes() and len(d) == 0 and d.ids.size == 0


def test_a_duplicate_on_a_tile_boundary(small, gpu_lib):
    """Equal sets put pair p at merged positions 2p and 2p + 1; one more id in front of a moves every a to an odd position
    and its equal b to the next even one — the last position of a tile and the first of the next, at every boundary.
    Swapped (the lone id in front of b) the pairs stay inside a tile; both orders and both operand orders are checked."""
    T = int(gpu_lib.cs_scope_ops_tile())
    run = np.arange(10, 10 + 2 * T, dtype=np.uint32)
    _check_sets(small, np.concatenate([_u32([3]), run]), run)
    # runs of equal ids around each boundary only, the rest disjoint: a holds odd ids, b even ids, except that near every
    # multiple of T (in merged positions) both hold the same 8 ids
    a = np.arange(1, 6 * T, 2, dtype=np.uint32)
    b = np.arange(0, 6 * T, 2, dtype=np.uint32)
    shared = np.concatenate([np.arange(k * T - 3, k * T + 5, dtype=np.uint32) for k in range(1, 6)])
    for lead in ([], [0]):
        aa = np.union1d(np.union1d(a, shared), _u32(lead)).astype(np.uint32)
        bb = np.union1d(b, shared).astype(np.uint32)
        for drop in range(3):  # shift the merged positions of everything behind by 0, 1, 2
            _check_sets(small, aa[drop:], bb)


def test_ids_zero_and_u32_max(small, gpu_lib):
    T = int(gpu_lib.cs_scope_ops_tile())
    top = 0xFFFFFFFF
    _check_sets(small, [0, 7, top], [0, top - 1, top])
    _check_sets(small, [0], [top])
    _check_sets(small, [top], [top])
    _check_sets(small, np.arange(top - (T + 2), top + 1, dtype=np.int64), np.arange(top - 2 * T, top + 1, 3, dtype=np.int64))


def test_two_million_ids_a_side(small):
    rng = np.random.default_rng(13)
    a = np.flatnonzero(rng.random(5_000_000) < 0.4).astype(np.uint32)
    b = np.flatnonzero(rng.random(5_000_000) < 0.4).astype(np.uint32)
    assert a.size > 1_900_000 and b.size > 1_900_000
    with small.scope(a) as sa, small.scope(b) as sb:
        for op in ("union", "intersection", "difference"):
            with getattr(sa, op)(sb) as got:
                assert got.ids.tobytes() == _host_op(op, a, b).tobytes(), op


def test_scope_range(small):
    top = 1 << 32
    for first, n in ((0, 0), (17, 0), (0, 1), (5, 4097), (990, 20), (top - 5000, 5000), (top - 1, 1), (top - 1, 0)):
        with small.scope_range(first, n) as r:
            assert len(r) == n and r.info()[0] == n
            assert r.ids.tobytes() == np.arange(first, first + n, dtype=np.int64).astype(np.uint32).tobytes(), (first, n)
    with small.scope_all() as every, small.scope(np.arange(1000)) as twin:
        assert every.ids.tobytes() == twin.ids.tobytes() and every.info() == twin.info()
    with small.scope_range(3, 100) as r:  # read_ids in pieces
        out = np.zeros(10, np.uint32)
        _lib.check(small._lib.cs_scope_read_ids(r.handle, 95, 5, out.ctypes.data_as(_lib.u32p)))
        assert out[:5].tolist() == [98, 99, 100, 101, 102] and not out[5:].any()
        _lib.check(small._lib.cs_scope_read_ids(r.handle, 100, 0, None))


# ---- 2. every scoped call ----------------------------------------------------------------------------------------------

def _rich_store(VS, n, dim, seed):
    """n rows in files of 8 with classes, one file of 60 near-duplicates (ids 200 .. 259) and some deleted rows."""
    rows = synth_rows(seed, 0, n, dim).copy()
    rng = np.random.default_rng(seed)
    rows[200:260] = rows[200] + 0.02 * rng.standard_normal((60, dim)).astype(np.float32) * np.abs(rows[200]).mean()
    st = VS(None, dim)
    st.insert_embeddings(rows)
    groups = np.arange(n, dtype=np.uint32) // 8
    groups[200:260] = 200 // 8
    st.set_groups(np.arange(n), groups)
    st.set_classes(np.arange(n), (np.arange(n) % 5).astype(np.uint16))
    dead = rng.choice(n, n // 50, replace=False)
    dead = dead[((dead < 200) | (dead >= 260)) & (dead != 5) & (dead != 777)]  # (5, 201, 777: the similar search's sources)
    st.delete_chunks(dead)
    st.build_index()
    return st, rows


def _answers(st, sc, queries, other=None, pairs=True):
    """Every scoped call through `sc`, as bytes."""
    out = {}

    def put(name, res):
        out[name] = tuple(x.tobytes() if isinstance(x, np.ndarray) else x for x in res)

    weights = np.array([1.0, 1.15, 0.9, 1.0, 1.3], np.float32)
    for route in ("gather", "filter", "auto"):
        sc.set_route(route)
        put("search/" + route, st.search_raw(queries, 10, scope=sc))
        put("search1/" + route, st.search_raw(queries[0], 10, scope=sc))
        put("variants/" + route, st.search_variants_raw(queries, 10, scope=sc))
        put("similar/" + route, st.similar_raw([5, 201, 777], 10, exclude="file", scope=sc))
    put("per_file", st.search_raw(queries[:3], 10, scope=sc, per_file=1))
    put("boosted", st.search_raw(queries[:3], 10, scope=sc, class_weights=weights))
    put("boosted_grouped_variants", st.search_variants_raw(queries, 10, scope=sc, per_file=1, class_weights=weights))
    if pairs:
        put("pairs", st.similar_pairs_raw(0.9, scope=sc))
        put("pairs_other", st.similar_pairs_raw(0.9, other_files=False, scope=sc, other=other))
        put("clusters", st.similar_clusters_raw(0.9, scope=sc))
        put("clusters_other", st.similar_clusters_raw(0.9, scope=sc, other=other))
    return out


def _same_answers(st, got_sc, twin_sc, queries, other=None, pairs=True):
    g = _answers(st, got_sc, queries, other, pairs)
    w = _answers(st, twin_sc, queries, other, pairs)
    assert g.keys() == w.keys()
    for k in w:
        assert g[k] == w[k], k
    assert got_sc.info()[:2] == twin_sc.info()[:2]
    assert got_sc.route_info() == twin_sc.route_info()  # the same routes taken, the same extra bytes held


def _four(st, A, B, a_ids, b_ids, every_ids):
    """(name, combined scope, twin's ids) of A|B, A&B, A-B and all-A."""
    with st.scope_all() as every:  # closed here: an input may go before its result is searched
        assert every.ids.tobytes() == _u32(every_ids).tobytes()
        rest = every - A
    return [("A|B", A | B, _host_op("union", a_ids, b_ids)), ("A&B", A & B, _host_op("intersection", a_ids, b_ids)),
            ("A-B", A - B, _host_op("difference", a_ids, b_ids)), ("all-A", rest, _host_op("difference", every_ids, a_ids))]


@pytest.mark.parametrize("n,dim,pairs", [(5000, 384, True), (1000, 100, False)])
def test_every_scoped_call_answers_as_the_twin(VS, n, dim, pairs):
    st, _ = _rich_store(VS, n, dim, 4200 + dim)
    rng = np.random.default_rng(n)
    a_ids = _random_set(rng, n * 7 // 10, n)
    b_ids = np.arange(n // 10, n // 10 + n * 4 // 10, dtype=np.uint32)
    queries = synth_rows(4300 + dim, 0, 9, dim)
    A, B = st.scope(a_ids), st.scope(b_ids)
    for name, got, want_ids in _four(st, A, B, a_ids, b_ids, np.arange(n)):
        twin = st.scope(want_ids)
        assert got.ids.tobytes() == want_ids.tobytes(), name
        _same_answers(st, got, twin, queries, other=B, pairs=pairs)
        if n == 5000 and name == "A|B":  # above 3,072 rows: the filter tables are kept, and the filter answered
            assert got.route_info()[3] > 0 and got.route_info()[0] > 0
        got.close()
        twin.close()
    A.close()
    B.close()
    st.close()


# ---- 3. life cycle -----------------------------------------------------------------------------------------------------

def test_life_cycle(VS):
    n, dim = 4000, 384
    rows = synth_rows(4400, 0, n + 600, dim)
    st = VS(None, dim)
    st.insert_embeddings(rows[:n])
    rng = np.random.default_rng(5)
    a_ids = _random_set(rng, 2800, n + 300)           # names ids not issued yet: they pass through
    b_ids = np.arange(400, 2000, dtype=np.uint32)
    queries = synth_rows(4401, 0, 9, dim)
    A, B = st.scope(a_ids), st.scope(b_ids)
    assert not st.is_indexed()
    made = [(name, got, st.scope(ids)) for name, got, ids in _four(st, A, B, a_ids, b_ids, np.arange(n))]  # store not built
    A.close()
    B.close()  # the inputs go before any result is searched
    for name, got, twin in made:
        assert got.info() == twin.info() == (len(twin), 0, 0), name

    def compare(step, refreshes):
        for name, got, twin in made:
            g = (st.search_raw(queries, 10, scope=got), st.search_variants_raw(queries, 10, scope=got))
            w = (st.search_raw(queries, 10, scope=twin), st.search_variants_raw(queries, 10, scope=twin))
            for x, y in zip(g[0] + g[1], w[0] + w[1]):
                assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y, (step, name)
            assert got.info() == twin.info(), (step, name, got.info(), twin.info())
            assert refreshes is None or got.info()[2] == refreshes, (step, name, got.info())

    st.build_index()
    compare("first build", 1)
    dead = np.concatenate([a_ids[a_ids < n][::4], b_ids[::3]])  # rows of both inputs, above a tenth of the store
    assert st.delete_chunks(np.unique(dead)) > n // 10
    st.build_index()  # a reclaiming build: the rows move
    assert st.stored_rows() == len(st)
    compare("delete + build", 2)
    st.insert_embeddings(rows[n:])  # ids n .. n + 599: some of them are in A
    st.build_index()
    compare("append + build", 3)
    st.clear()
    for name, got, twin in made:
        outcome = []
        for sc in (got, twin):
            try:
                res = st.search_raw(queries, 10, scope=sc)
                outcome.append(tuple(x.tobytes() for x in res))
            except _lib.CsError as e:
                outcome.append((e.code, str(e)))
        assert outcome[0] == outcome[1], ("clear", name)
        assert got.info() == twin.info(), ("clear", name)
    st.insert_embeddings(rows[:500])
    st.build_index()
    compare("refill + build", None)
    st.close()


# ---- 4. sharded ----------------------------------------------------------------------------------------------------------

def test_sharded_scopes_combine_part_by_part(VS):
    n, dim = 1000, 384
    st = VS(None, dim, devices=[0, 0, 0], rows_per_stripe=64)
    st.insert_embeddings(synth_rows(4500, 0, n, dim))
    st.build_index()
    rng = np.random.default_rng(6)
    a_ids = _random_set(rng, 700, n + 50)
    b_ids = np.arange(100, 500, dtype=np.uint32)
    queries = synth_rows(4501, 0, 9, dim)
    A, B = st.scope(a_ids), st.scope(b_ids)
    cases = _four(st, A, B, a_ids, b_ids, np.arange(n))
    cases.append(("range", st.scope_range(130, 333), np.arange(130, 463, dtype=np.uint32)))
    cases.append(("range0", st.scope_range(64, 0), np.zeros(0, np.uint32)))
    for name, got, want_ids in cases:
        assert got.ids.tobytes() == want_ids.tobytes(), name  # global ids, ascending
        assert len(got) == want_ids.size
        with st.scope(want_ids) as twin:
            for x, y in zip(st.search_raw(queries, 10, scope=got) + st.search_variants_raw(queries, 10, scope=got),
                            st.search_raw(queries, 10, scope=twin) + st.search_variants_raw(queries, 10, scope=twin)):
                assert (x.tobytes() == y.tobytes()) if isinstance(x, np.ndarray) else x == y, name
            assert got.info() == twin.info(), name
        got.close()
    # read_ids in the middle of a sharded scope
    with st.scope(a_ids) as a2:
        out = np.zeros(100, np.uint32)
        _lib.check(st._lib.cs_scope_read_ids(a2.handle, 300, 100, out.ctypes.data_as(_lib.u32p)))
        assert out.tobytes() == a_ids[300:400].tobytes()
    st.close()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------

def test_refusals(VS, small, gpu_lib):
    lib = gpu_lib
    BAD = _lib.CS_ERR_BAD_ARG
    other = VS(None, 384)
    other.insert_embeddings(synth_rows(4600, 0, 64, 384))
    sharded = VS(None, 384, devices=[0, 0], rows_per_stripe=16)
    sharded.insert_embeddings(synth_rows(4601, 0, 64, 384))
    sharded2 = VS(None, 384, devices=[0, 0], rows_per_stripe=16)
    small.set_groups([1, 2, 3], [7, 7, 8])
    a, b = small.scope([1, 2, 3, 900]), small.scope([2, 3, 4])
    o, s, s2 = other.scope([1, 2]), sharded.scope([1, 2, 40]), sharded2.scope([1])
    before = (a.info(), b.info(), a.route_info(), b.route_info(), small.groups_info())

    def refused(status, text):
        assert status == BAD, status
        assert text in _lib.last_error(), _lib.last_error()

    out = C.c_void_p(0xDEAD)
    refused(lib.cs_scope_combine(a.handle, b.handle, 0, None), "out is null")
    for args, text in (((None, b.handle, 0), "null scope handle (a)"), ((a.handle, None, 0), "null scope handle (b)"),
                       ((None, None, 9), "null scope handle (a)"),
                       ((a.handle, b.handle, 3), "op must be CS_SCOPE_OP_UNION, _INTERSECT or _DIFFERENCE, got 3"),
                       ((a.handle, b.handle, -1), "got -1"),
                       ((a.handle, o.handle, 0), "the scopes were made for different stores"),
                       ((s.handle, s2.handle, 1), "the scopes were made for different stores"),
                       ((a.handle, s.handle, 2), "one over an index, one over a sharded store"),
                       ((s.handle, a.handle, 2), "one over an index, one over a sharded store")):
        out.value = 0xDEAD
        refused(lib.cs_scope_combine(*args, C.byref(out)), text)
        assert not out.value, args  # *out is NULL afterwards
    for fn, h in ((lib.cs_index_scope_create_range, small._h), (lib.cs_shards_scope_create_range, sharded._h)):
        refused(fn(h, 0, 5, None), "out is null")
        for args, text in (((None, 0, 5), "handle"), ((h, 2, 0xFFFFFFFF), "ends past 2^32"), ((h, 0xFFFFFFFF, 2), "ends past 2^32"),
                           ((h, 0, 1 << 32), "at most 2^32 - 1 ids")):
            out.value = 0xDEAD
            refused(fn(*args, C.byref(out)), text)
            assert not out.value, args
    buf = np.zeros(8, np.uint32)
    p = buf.ctypes.data_as(_lib.u32p)
    refused(lib.cs_scope_read_ids(None, 0, 1, p), "null scope handle")
    refused(lib.cs_scope_read_ids(a.handle, 3, 2, p), "ids [3, 5) asked of a scope of 4 ids")
    refused(lib.cs_scope_read_ids(a.handle, 5, 0, p), "asked of a scope of 4 ids")
    refused(lib.cs_scope_read_ids(s.handle, 0, 4, p), "asked of a scope of 3 ids")
    refused(lib.cs_scope_read_ids(a.handle, 0, 4, None), "null buffer")
    assert not buf.any()
    # Python: the library's error for another store's scope, "scope is closed" for a closed one, TypeError for no scope
    with pytest.raises(_lib.CsError, match="different stores") as e:
        a | o
    assert e.value.code == BAD
    with pytest.raises(TypeError):
        a | [1, 2]
    c = small.scope([5])
    c.close()
    for f in (lambda: a | c, lambda: c - a, lambda: c & c, lambda: c.info()):
        with pytest.raises(_lib.CsError, match="scope is closed"):
            f()
    with pytest.raises(ValueError):
        small.scope_range(-1, 3)
    assert (a.info(), b.info(), a.route_info(), b.route_info(), small.groups_info()) == before  # the inputs are untouched
    u = a | b
    assert u.store is small and u in small._scopes and u.ids.tolist() == [1, 2, 3, 4, 900]  # registered like any scope
    other.close()
    sharded.close()
    sharded2.close()
    assert o._h is None and s._h is None  # closed with their stores
    u.close()
    a.close()
    b.close()
    small.set_groups([1, 2, 3], [0xFFFFFFFF] * 3)


def _read(sc, first, n):
    out = np.zeros(n, np.uint32)
    _lib.check(sc.store._lib.cs_scope_read_ids(sc.handle, first, n, out.ctypes.data_as(_lib.u32p)))
    return out.astype(np.int64)


def test_a_result_of_every_u32_id_is_refused(VS, small, gpu_lib):
    """A scope holds at most 2^32 - 1 ids, so the one result that cannot exist is the union that names every u32 id.  The
    fault can show only at this size — 2^32 merged positions, 2^20 tiles, per-tile u32 counts whose scan wraps to exactly 0 —
    so the test runs it: a range scope of [0, 2^32 - 1) needs no host list (8 B per id: 32 GiB of HBM, 64 GiB while the
    boundary case beside it, a union of exactly 2^32 - 1 ids, holds its result)."""
    lib, BAD, top = gpu_lib, _lib.CS_ERR_BAD_ARG, 0xFFFFFFFF
    T = int(lib.cs_scope_ops_tile())
    text = "a scope holds at most 2^32 - 1 ids"
    queries = synth_rows(4650, 0, 2, 384)
    with small.scope_range(0, top) as low, small.scope([top]) as last, small.scope([5, 77]) as inside:
        assert len(low) == top and low.info()[:2] == (top, 1000)
        before = (low.info(), last.info(), low.route_info(), last.route_info())
        for x, y in ((low, last), (last, low)):
            out = C.c_void_p(0xDEAD)
            assert lib.cs_scope_combine(x.handle, y.handle, 0, C.byref(out)) == BAD
            assert text in _lib.last_error(), _lib.last_error()
            assert not out.value  # *out is NULL afterwards
        with pytest.raises(_lib.CsError, match=r"at most 2\^32 - 1 ids") as e:
            low | last
        assert e.value.code == BAD
        assert (low.info(), last.info(), low.route_info(), last.route_info()) == before  # the inputs are untouched
        # the other operations of the same two inputs exist
        with low & last as none, last - low as only:
            assert len(none) == 0 and only.ids.tolist() == [top]
        # the boundary: a union of exactly 2^32 - 1 ids succeeds and is the range (one operand order: each such scope
        # costs about a second to allocate and list)
        with low | inside as u:
            assert len(u) == top and u.info()[:2] == low.info()[:2]
            for first in (0, T - 2, (1 << 31) - 3, (1 << 32) - 2 * T - 3, top - 6):
                assert _read(u, first, 6).tolist() == list(range(first, first + 6)), first
            for a, b in zip(small.search_raw(queries, 10, scope=u), small.search_raw(queries, 10, scope=low)):
                assert a.tobytes() == b.tobytes()
    # sharded: every part's union exists, their sum does not
    sharded = VS(None, 384, devices=[0, 0], rows_per_stripe=64)
    with sharded.scope_range(0, top) as low, sharded.scope([top]) as last:
        assert len(low) == top
        before = (low.info(), last.info())
        out = C.c_void_p(0xDEAD)
        assert lib.cs_scope_combine(low.handle, last.handle, 0, C.byref(out)) == BAD
        assert text in _lib.last_error() and not out.value
        assert (low.info(), last.info()) == before
        with last - low as only:
            assert only.ids.tolist() == [top]
    sharded.close()


# ---- 6. concurrency ------------------------------------------------------------------------------------------------------

def test_combining_beside_searches(VS):
    n, dim = 4000, 384
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(4700, 0, n, dim))
    st.build_index()
    rng = np.random.default_rng(7)
    a_ids, b_ids = _random_set(rng, 2500, n), _random_set(rng, 2000, n)
    queries = synth_rows(4701, 0, 4, dim)
    A, B = st.scope(a_ids), st.scope(b_ids)
    want_sets = {op: _host_op(op, a_ids, b_ids).tobytes() for op in NUMPY_OPS}
    want_search = {"A": tuple(x.tobytes() for x in st.search_raw(queries, 10, scope=A)),
                   "B": tuple(x.tobytes() for x in st.search_raw(queries, 10, scope=B))}
    with A | B as u:
        want_union = tuple(x.tobytes() for x in st.search_raw(queries, 10, scope=u))
    errors = []

    def combiner(i):
        try:
            for r in range(6):
                op = list(NUMPY_OPS)[(i + r) % 3]
                with getattr(A, op)(B) as got:
                    assert got.ids.tobytes() == want_sets[op], op
                    if op == "union":
                        assert tuple(x.tobytes() for x in st.search_raw(queries, 10, scope=got)) == want_union
        except Exception as e:  # noqa: BLE001 — reported by the main thread
            errors.append(repr(e))

    def searcher(i):
        try:
            for r in range(12):
                name, sc = (("A", A), ("B", B))[(i + r) % 2]
                assert tuple(x.tobytes() for x in st.search_raw(queries, 10, scope=sc)) == want_search[name], name
        except Exception as e:  # noqa: BLE001
            errors.append(repr(e))

    threads = [threading.Thread(target=combiner, args=(i,)) for i in range(4)] + \
              [threading.Thread(target=searcher, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    st.close()


# ---- the C++ mirror --------------------------------------------------------------------------------------------------------

def test_cpp_host_mirror_scope_algebra(gpu_lib):
    """host/codesearch_gpu.hpp: Scope::combine, Scope::read_ids and VectorStore::scope_range over one index and over a
    sharded store (tests/cpp/scope_algebra_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "scope_algebra_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "scope_algebra_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "scope algebra host ok" in r.stdout
