"""Search scopes (cs_index_scope_create, cs_index_search_scoped & co.; codesearch_amd/csrc/scan_masked.hip part 4): a
prepared set of chunk ids that lives on the device and is searched any number of times.

The one bar: a scoped search returns, byte for byte (cosines, ids, counts, the variants' count and flag), what the masked
search of the same store returns at that moment for a bitmap of exactly the scope's ids — for every dim path, mask shape,
k and query count, at every block edge of the id-list pass, and through builds, deletes (tombstoning and reclaiming),
appends and clear; over the sharded store; from several threads; and through the device-pointer form."""
import ctypes as C
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd._lib import f32p, u32p
from codesearch_amd.synth import synth_rows
from tests.test_gpu_masked_search import _masks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _equals_masked(st, sc, qs, k):
    """search_raw(scope=) against search_raw(chunk_ids=) of the scope's ids -> the (shared) answer."""
    a = st.search_raw(qs, k, scope=sc)
    b = st.search_raw(qs, k, chunk_ids=sc.ids)
    assert _same(a, b), (len(sc), k, qs.shape[0])
    return a


def _store(VS, n, dim, seed, **kw):
    st = VS(None, dim, **kw)
    rows = synth_rows(seed, 0, n, dim)
    ids = st.insert_embeddings(rows)
    st.build_index()
    return st, rows, ids


SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1024, 16), (10, 40)]  # (k, nq)


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_scoped_equals_masked(VS, dim):
    rng = np.random.default_rng(dim)
    n, seed = 12_000, 8100 + dim
    st, rows, _ = _store(VS, n, dim, seed)
    qs = np.concatenate([synth_rows(seed + 1, 0, 38, dim), rows[[5, n - 3]]])
    for name, allowed in _masks(n, rng).items():
        with st.scope(allowed) as sc:
            assert sc.info() == (allowed.size, allowed.size, 1), name
            for k, nq in SHAPES:
                c, i, cnt = _equals_masked(st, sc, qs[:nq], k)
                assert cnt.tolist() == [min(k, allowed.size)] * nq
                if allowed.size:
                    assert set(i[0][:cnt[0]].tolist()) <= set(allowed.tolist())
    st.close()


@pytest.mark.parametrize("layout", ["contiguous", "strided"])
def test_block_edges_of_the_id_list_pass(VS, layout):
    """One wave, one 256-id step and one 4,096-id block of the id-list pass, each at -1 / 0 / +1, and three blocks."""
    n, dim, k = 20_000, 384, 10
    st, rows, _ = _store(VS, n, dim, 0xED6E)
    qs = synth_rows(0xED6F, 0, 2, dim)
    for size in (1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193):
        ids = np.arange(1234, 1234 + size) if layout == "contiguous" else 3 + 2 * np.arange(size)
        with st.scope(ids) as sc:
            assert sc.info() == (size, size, 1)
            c, i, cnt = _equals_masked(st, sc, qs, k)
            assert cnt.tolist() == [min(k, size)] * 2 and set(i[0][:cnt[0]].tolist()) <= set(ids.tolist())
            if size > k:  # a row of the scope's last entry is found: the list's tail is there
                assert st.search_raw(rows[ids[-1]], 1, scope=sc)[1][0][0] == ids[-1]
    st.close()


def test_life_cycle(VS):
    n, dim, k, base = 20_000, 384, 50, 1_000_000
    st, rows, ids = _store(VS, n, dim, 0x11FE, id_base=base)
    assert ids[0] == base
    rng = np.random.default_rng(17)
    # (rows 100.. only: after clear() the store issues ids base .. base + 99 again, and the scope is to match none of them)
    rows_in = np.sort(rng.choice(np.arange(100, n), 4000, replace=False))
    qs = np.concatenate([synth_rows(0x11FF, 0, 3, dim), rows[rows_in[:2]]])
    sc = st.scope(rows_in + base)
    future = st.scope(np.concatenate([rows_in[:200] + base, base + n + 10 + np.arange(50)]))  # 50 ids >= next_id
    below = st.scope(np.arange(base - 500, base))
    assert sc.info() == (4000, 4000, 1) and future.info() == (250, 200, 1) and below.info() == (500, 0, 1)
    first = _equals_masked(st, sc, qs, k)
    for _ in range(100):
        assert _same(st.search_raw(qs[:1], k, scope=sc), [x[:1] for x in first])
    assert sc.info() == (4000, 4000, 1)
    _equals_masked(st, future, qs, k)
    c, i, cnt = _equals_masked(st, below, qs, k)
    assert cnt.tolist() == [0] * 5 and (i == 0xFFFFFFFF).all()

    # tombstones: 300 ids of the scope, 1.5 % of the rows -> no reclaim
    dead = np.sort(rng.choice(rows_in, 300, replace=False))
    st.delete_chunks((dead + base).tolist())
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.search_raw(qs, k, scope=sc)
    st.build_index()
    assert st.stored_rows() == n
    c1, i1, n1 = _equals_masked(st, sc, np.concatenate([qs, rows[dead[:2]]]), k)
    assert not (set(i1.ravel().tolist()) & set((dead + base).tolist()))
    assert sc.info() == (4000, 3700, 2)
    _equals_masked(st, sc, qs, k)
    assert sc.info()[2] == 2  # the same generation again: no refresh

    # a reclaiming build: the row -> id table exists from here on, the id-list pass bisects it
    more = np.setdiff1d(np.arange(n), rows_in)[:3000]
    st.delete_chunks((more + base).tolist())
    st.build_index()
    assert st.stored_rows() == n - 3300
    c2, i2, n2 = _equals_masked(st, sc, np.concatenate([qs, rows[dead[:2]]]), k)
    assert c2.tobytes() == c1.tobytes() and i2.tobytes() == i1.tobytes() and n2.tolist() == n1.tolist()
    assert sc.info() == (4000, 3700, 3)
    c, i, cnt = _equals_masked(st, below, qs, k)
    assert cnt.tolist() == [0] * 5
    # a scope made on the compacted index, with ids of reclaimed rows in it
    with st.scope(np.concatenate([more[:500], rows_in[:500]]) + base) as mixed:
        assert mixed.info()[1] == 500 - np.intersect1d(rows_in[:500], dead).size
        _equals_masked(st, mixed, qs, k)

    # an append issues the ids `future` was waiting for
    c, i, cnt = _equals_masked(st, future, qs, k)
    assert not (set(i.ravel().tolist()) & set((base + n + 10 + np.arange(50)).tolist()))
    new_rows = synth_rows(0x1200, 0, 5000, dim)
    new_ids = st.insert_embeddings(new_rows)
    assert new_ids[0] == base + n
    st.build_index()
    _equals_masked(st, sc, qs, k)
    c, i, cnt = _equals_masked(st, future, new_rows[10:12], 5)
    assert i[:, 0].tolist() == [base + n + 10, base + n + 11]
    assert future.info()[1] == 200 - np.intersect1d(rows_in[:200], dead).size + 50

    # clear(): the ids start over at id_base; the scopes match what is issued again, here nothing
    st.clear()
    st.insert_embeddings(rows[:100])
    st.build_index()
    for s in (sc, future, below):
        c, i, cnt = _equals_masked(st, s, qs, k)
        assert cnt.tolist() == [0] * 5 and (i == 0xFFFFFFFF).all()
        assert s.info()[1] == 0
    with st.scope(base + np.arange(50, 150)) as again:  # ... and a scope over the reissued ids finds them
        c, i, cnt = _equals_masked(st, again, qs, k)
        assert cnt.tolist() == [50] * 5
    for s in (sc, future, below):
        s.close()
    st.close()


def _scope_create(lib, fn, handle, ids):
    ids = np.ascontiguousarray(ids, np.uint32)
    h = C.c_void_p()
    _lib.check(fn(handle, ids.ctypes.data_as(u32p) if ids.size else None, ids.size, C.byref(h)))
    return h


def test_arguments(VS, gpu_lib):
    st = VS(None, 384)
    st.insert_synthetic(1000, 1, 0)
    q = synth_rows(2, 0, 1, 384)
    sc = st.scope([1, 2])  # made before the first build: the first search makes the list
    assert sc.info() == (2, 0, 0)
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.search_raw(q, 5, scope=sc)
    st.build_index()
    with pytest.raises(_lib.CsError, match="Query embedding dimension mismatch: expected 384, got 100"):
        st.search_raw(np.zeros((1, 100), np.float32), 5, scope=sc)
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 0"):
        st.search_raw(q, 0, scope=sc)
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 1025"):
        st.search_raw(q, 1025, scope=sc)
    with pytest.raises(_lib.CsError, match="at most 16 query variants"):
        st.search_variants(np.zeros((17, 384), np.float32), 5, scope=sc)
    assert sc.info() == (2, 0, 0)  # none of them got as far as the list
    c, i, cnt = st.search_raw(q, 5, scope=sc)
    assert cnt.tolist() == [2] and sorted(i[0][:2].tolist()) == [1, 2] and sc.info() == (2, 2, 1)

    # the id list: strictly ascending, and the message carries the first offending position
    for bad, pos in (([5, 9, 7, 3], 2), ([5, 9, 9, 12], 2), ([3, 3], 1)):
        with pytest.raises(_lib.CsError, match=rf"strictly ascending: ids\[{pos}\]") as e:
            _scope_create(gpu_lib, gpu_lib.cs_index_scope_create, st.handle, bad)
        assert e.value.code == _lib.CS_ERR_BAD_ARG
    # VectorStore.scope sorts and de-duplicates for the caller
    with st.scope([9, 5, 9, -4, 7]) as tidy:
        assert tidy.ids.tolist() == [5, 7, 9] and tidy.info() == (3, 3, 1)

    # the empty scope: success, nothing found
    with st.scope([]) as empty:
        assert empty.info() == (0, 0, 1)
        c, i, cnt = st.search_raw(q, 5, scope=empty)
        assert cnt.tolist() == [0] and (i == 0xFFFFFFFF).all() and (c == 0).all()
        res, flag = st.search_variants(q, 5, scope=empty)
        assert res == [] and flag is False

    # a scope of store A on store B
    other = VS(None, 384)
    other.insert_synthetic(1000, 1, 0)
    other.build_index()
    with pytest.raises(_lib.CsError, match="made for another store") as e:
        other.search_raw(q, 5, scope=sc)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    with pytest.raises(_lib.CsError, match="made for another store"):
        other.search_variants(q, 5, scope=sc)
    with pytest.raises(ValueError, match="exclusive"):
        st.search_raw(q, 5, chunk_ids=[1], scope=sc)
    # closing a store closes its scopes first; a closed scope is refused, not dereferenced
    other.close()
    st.close()
    assert sc.handle is None
    with pytest.raises(_lib.CsError, match="scope is closed"):
        sc.info()


def _raw_variants(store, qs, k, scope=None, chunk_ids=None):
    from codesearch_amd.vector_store import allow_mask

    cos = np.zeros(k, np.float32)
    ids = np.zeros(k, np.uint32)
    cnt, fl = C.c_uint32(), C.c_int32()
    if scope is not None:
        _lib.check(store._fn("search_variants_scoped")(store._h, scope.handle, qs.ctypes.data_as(f32p), qs.shape[0],
                                                       qs.shape[1], k, cos.ctypes.data_as(f32p), ids.ctypes.data_as(u32p),
                                                       C.byref(cnt), C.byref(fl)))
    else:
        nxt = store.next_id()
        mask = allow_mask(chunk_ids, nxt)
        _lib.check(store._fn("search_variants_masked")(store._h, qs.ctypes.data_as(f32p), qs.shape[0], qs.shape[1], k,
                                                       mask.ctypes.data_as(u32p) if mask.size else None,
                                                       nxt if mask.size else 0, cos.ctypes.data_as(f32p),
                                                       ids.ctypes.data_as(u32p), C.byref(cnt), C.byref(fl)))
    return cos.tobytes(), ids.tobytes(), cnt.value, fl.value


def test_scoped_variants_equal_masked_variants(VS):
    n, dim, k, seed = 30_000, 384, 200, 0x7A8
    st, rows, _ = _store(VS, n, dim, seed)
    rng = np.random.default_rng(5)
    allowed = np.sort(rng.choice(n, 3000, replace=False))
    near = rows[allowed[11]]  # nine variants of one query near an allowed row: a confident answer
    qs = np.stack([near + 0.01 * synth_rows(seed + 2 + v, 0, 1, dim)[0] for v in range(9)]).astype(np.float32)
    far = synth_rows(seed + 40, 0, 9, dim)
    with st.scope(allowed) as sc:
        for q in (qs, far, qs[:1]):
            a = _raw_variants(st, q, k, scope=sc)
            b = _raw_variants(st, q, k, chunk_ids=allowed)
            assert a == b
        assert _raw_variants(st, qs, k, scope=sc)[2] == k
    st.close()


@pytest.mark.parametrize("stripe", [1, 100, 4096])
def test_shards_scoped_equal_single_index(VS, stripe):
    n, dim, seed = 40_000, 384, 0x5A4E
    rows = synth_rows(seed, 0, n, dim)
    one = VS(None, dim)
    one.insert_embeddings(rows)
    sh = VS(None, dim, devices=[0] * 8, rows_per_stripe=stripe)
    sh.insert_embeddings(rows)
    rng = np.random.default_rng(stripe)
    gone = rng.choice(n, 500, replace=False)
    one.delete_chunks(gone.tolist())
    sh.delete_chunks(gone.tolist())
    one.build_index()
    sh.build_index()
    qs = synth_rows(seed + 1, 0, 5, dim)
    unscoped = sh.search_raw(qs, 10)
    for allowed in (np.arange(10_000, 14_000), np.sort(rng.choice(n, 2000, replace=False)), np.array([77, 30_001]),
                    np.zeros(0, np.int64)):
        with one.scope(allowed) as s1, sh.scope(allowed) as s8:
            live = np.setdiff1d(allowed, gone).size
            assert s1.info() == (allowed.size, live, 1) and s8.info()[:2] == (allowed.size, live)
            for k in (10, 200):
                a = _equals_masked(one, s1, qs, k)
                b = _equals_masked(sh, s8, qs, k)
                assert _same(a, b), (stripe, allowed.size, k)
            assert _raw_variants(one, qs, 50, scope=s1) == _raw_variants(sh, qs, 50, scope=s8)
            assert _raw_variants(sh, qs, 50, scope=s8) == _raw_variants(sh, qs, 50, chunk_ids=allowed)
    with one.scope([1, 2]) as s1:  # a single index's scope on the sharded store
        with pytest.raises(_lib.CsError, match="made for another store"):
            sh.search_raw(qs, 10, scope=s1)
    # unscoped shard searches are untouched by the scoped ones in between
    assert _same(unscoped, sh.search_raw(qs, 10)) and _same(unscoped, one.search_raw(qs, 10))
    one.close()
    sh.close()


def test_concurrent_scopes_on_one_store(VS):
    n, dim, k = 60_000, 384, 25
    st = VS(None, dim)
    st.insert_synthetic(n, 0xC0C2, 0)
    st.build_index()
    q = synth_rows(0xC0C3, 0, 2, dim)
    before = st.search_raw(q, k)
    counters = st.debug_counters()
    masks = [np.arange(t * 6000, t * 6000 + 5000) for t in range(9)]
    scopes = [st.scope(m) for m in masks]
    owner = list(range(8)) + [8, 8]  # eight threads with a scope each, two more share the ninth

    def round_(want):
        errors = []

        def work(t):
            try:
                for _ in range(6):
                    if not _same(st.search_raw(q, k, scope=scopes[owner[t]]), want[owner[t]]):
                        errors.append(t)
            except Exception as e:  # pragma: no cover - reported below
                errors.append(repr(e))

        th = [threading.Thread(target=work, args=(t,)) for t in range(10)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors

    want = [st.search_raw(q, k, chunk_ids=m) for m in masks]
    round_(want)
    assert [s.info()[2] for s in scopes] == [1] * 9
    assert st.debug_counters() == counters  # scoped searches leave the batched-path counters alone
    # a delete and a build with no thread running: every scope refreshes once, the shared one too
    st.delete_chunks(np.arange(100, 60_000, 50).tolist())
    st.build_index()
    want = [st.search_raw(q, k, chunk_ids=m) for m in masks]
    round_(want)
    assert [s.info()[2] for s in scopes] == [2] * 9
    assert scopes[8].info()[1] == 5000 - 100
    assert st.debug_counters() == counters
    st.close()
    assert before[0].shape == (2, k)


def test_device_pointer_form(VS, gpu_lib):
    import torch

    from codesearch_amd.sharded import key_unpack

    n, dim, k, nq = 20_000, 384, 20, 3
    st, rows, _ = _store(VS, n, dim, 0xDE71)
    qs = synth_rows(0xDE72, 0, nq, dim)
    allowed = np.sort(np.random.default_rng(9).choice(n, 2500, replace=False))
    vp = lambda t: C.c_void_p(t.data_ptr())
    d_q = torch.from_numpy(qs).to("cuda:0")
    stream = torch.cuda.Stream()
    for ids in (allowed, np.zeros(0, np.int64)):
        with st.scope(ids) as sc:
            want = st.search_raw(qs, k, scope=sc)
            keys = torch.full((nq, k), 7, dtype=torch.int64, device="cuda:0")
            cos = torch.full((nq, k), 7.0, dtype=torch.float32, device="cuda:0")
            out = torch.full((nq, k), 7, dtype=torch.int32, device="cuda:0")
            cnt = torch.full((nq,), 7, dtype=torch.int32, device="cuda:0")
            stream.wait_stream(torch.cuda.current_stream())
            _lib.check(gpu_lib.cs_index_search_scoped_device(st.handle, sc.handle, vp(d_q), nq, dim, k, vp(keys), vp(cos),
                                                            vp(out), vp(cnt), C.c_void_p(stream.cuda_stream)))
            stream.synchronize()
            kk = keys.cpu().numpy().view(np.uint64)
            filled = kk != 0
            kc, ki = key_unpack(kk)
            assert filled.sum(axis=1).tolist() == want[2].tolist()
            assert kc[filled].tobytes() == want[0][filled].tobytes() and ki[filled].tolist() == want[1][filled].tolist()
            assert cos.cpu().numpy().tobytes() == want[0].tobytes()
            assert out.cpu().numpy().view(np.uint32).tolist() == want[1].tolist()
            assert cnt.cpu().numpy().view(np.uint32).tolist() == want[2].tolist()
            assert sc.info()[2] == 1
    _lib.check(gpu_lib.cs_index_release_stream(st.handle, C.c_void_p(stream.cuda_stream)))
    st.close()


def test_scope_cache_serves_a_filter_path(VS):
    """search.vector_search_step narrows to a directory through a ScopeCache: one scope per filter_path, reused."""
    from codesearch_amd import Chunk, EmbeddedChunk
    from codesearch_amd.search import ScopeCache, vector_search_step

    n, dim = 3000, 384
    rows = synth_rows(0xCA, 0, n, dim)
    st = VS(None, dim)
    st.insert_chunks([EmbeddedChunk(Chunk(f"c{i}", 1, 2, "Function", f"src/d{i // 500}/f{i % 7}.rs"), rows[i]) for i in range(n)])
    st.build_index()
    qs = rows[[1200, 1300]] + 0.01 * synth_rows(0xCB, 0, 2, dim)
    cache = ScopeCache(st)
    want = vector_search_step(st, qs, 10, "src/d2")
    for _ in range(3):
        got = vector_search_step(st, qs, 10, "src/d2", scopes=cache)
        assert got == want and all(r.path.startswith("src/d2/") for r in got[0])
    assert len(cache) == 1 and cache.get("src/d2").info() == (500, 500, 1)
    cache.invalidate()
    assert len(cache) == 0
    st.close()
