"""cs_shards_search_grouped & co. — the grouped search (at most per_group hits per file, exact) over the row-sharded store
of one process.  The truth is the single-index call of the same name on a plain VectorStore holding the same rows, ids and
groups: cosine bits, ids, counts, count and flag are compared with np.array_equal.  One GPU is enough: N shards placed on
device 0 run the same code as N devices (streams, gather slots, event waits, the id remap and the cap in the root's merge).
Needs an MI355X."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, cap_per_group
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

f32p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_uint32)


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _pair(VS, rows, shards, stripe):
    """The same rows, built, in one index and in `shards` shards on device 0."""
    single = VS(None, rows.shape[1])
    sh = VS(None, rows.shape[1], devices=[0] * shards, rows_per_stripe=stripe, grouped=True)
    for st in (single, sh):
        assert st.insert_embeddings(rows).tolist() == list(range(len(rows)))
        st.build_index()
    assert sh.sharded
    return single, sh


def _set(stores, ids, groups):
    for st in stores:
        st.set_groups(ids, groups)


def _layout(name, n, seed):
    """Files of 8 consecutive ids, or 5 groups in all; a random 30 % of the ids without a group."""
    g = (np.arange(n) // 8 if name == "files" else np.arange(n) % 5).astype(np.uint32)
    g[np.random.default_rng(seed).random(n) < 0.3] = NO_GROUP
    return g


def _same(a, b):
    """Two raw answers, bit for bit: (cos, ids, counts) or (cos, ids, count, flag)."""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x, y = np.asarray(x), np.asarray(y)
        if x.dtype == np.float32:
            x, y = x.view(np.uint32), y.view(np.uint32)
        assert np.array_equal(x, y), (x, y)


def _queries(rows, seed, nq):
    """Random queries, the last one planted next to a stored row."""
    q = synth_rows(seed, 0, nq, rows.shape[1])
    q[-1] = rows[len(rows) // 3] + 0.05 * q[-1]
    return q


# ---- 1. equality --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
@pytest.mark.parametrize("shards,stripe", [(1, 100), (3, 1), (4, 7), (4, 1000), (3, 50_001)])
def test_sharded_grouped_equals_the_single_index(VS, dim, shards, stripe):
    n = 2003
    rows = synth_rows(7100 + dim, 0, n, dim)
    single, sh = _pair(VS, rows, shards, stripe)
    if stripe > n:
        assert sh.shard_lens() == [n] + [0] * (shards - 1)  # two shards hold nothing
    for layout in ("files", "five"):
        _set((single, sh), np.arange(n), _layout(layout, n, 5))
        assert sh.groups_info()[0] == single.groups_info()[0]
        for nq in (1, 9):
            q = _queries(rows, 7200 + nq, nq)
            for k in (1, 10, 200):
                for m in (1, 3):
                    _same(sh.search_raw(q, k, per_file=m), single.search_raw(q, k, per_file=m))
    sh.close(); single.close()


# ---- 2. the hog ----------------------------------------------------------------------------------------------------------

def test_a_file_of_near_duplicates_spread_over_all_shards(VS):
    """600 near-duplicates of the query in one group, dealt over four shards: every shard's capped list holds one of them,
    the root caps again, and ten groups answer.  Capping the uncapped list of ten on the host keeps one row."""
    n, dim, k = 3000, 384, 10
    rows = synth_rows(7301, 0, n, dim)
    q = synth_rows(7302, 0, 1, dim)
    rows[:600] = q[0] + 0.02 * rows[:600]
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    groups[:600] = 0
    single, sh = _pair(VS, rows, 4, 7)
    assert min(sh.shard_lens()) > 600 // 4 - 8
    _set((single, sh), np.arange(n), groups)
    got = sh.search_raw(q, k, per_file=1)
    _same(got, single.search_raw(q, k, per_file=1))
    assert int(got[2][0]) == k and len(set(groups[got[1][0]].tolist())) == k and groups[got[1][0][0]] == 0
    plain = sh.search_raw(q, k)
    assert set(groups[plain[1][0]].tolist()) == {0}
    kept = cap_per_group(plain[0][0], plain[1][0], groups[plain[1][0]], k, 1)
    assert len(kept[1]) == 1  # rank, then cap: nine of the ten places are lost
    sh.close(); single.close()


# ---- 3. two merge levels at the root -------------------------------------------------------------------------------------

@pytest.mark.parametrize("shards", [8, 4])  # 8,192 keys at the root: two levels; 4,096: exactly one block
def test_k_1024_over_eight_and_four_shards(VS, shards):
    n, dim, k = 5000, 384, 1024
    rows = synth_rows(7400, 0, n, dim)
    single, sh = _pair(VS, rows, shards, 100)
    _set((single, sh), np.arange(n), (np.arange(n) // 8).astype(np.uint32))
    for nq in (1, 3):
        q = _queries(rows, 7401 + nq, nq)
        got = sh.search_raw(q, k, per_file=2)
        _same(got, single.search_raw(q, k, per_file=2))
        assert got[2].tolist() == [k] * nq
    sh.close(); single.close()


# ---- 4. ties ---------------------------------------------------------------------------------------------------------------

def test_equal_cosines_in_different_shards_go_by_global_id(VS):
    half, dim = 1000, 384
    base = synth_rows(7500, 0, half, dim)
    rows = np.concatenate([base, base])  # id i and id i + 1000 are one vector
    stripe, shards = 7, 4
    shard_of = (np.arange(2 * half) // stripe) % shards
    assert (shard_of[:half] != shard_of[half:]).all()  # the two copies never share a shard
    groups = np.concatenate([np.arange(half) // 8, 500 + np.arange(half) // 8]).astype(np.uint32)
    single, sh = _pair(VS, rows, shards, stripe)
    _set((single, sh), np.arange(2 * half), groups)
    q = _queries(rows, 7501, 5)
    for k, m in ((10, 1), (64, 1), (200, 3)):
        got = sh.search_raw(q, k, per_file=m)
        _same(got, single.search_raw(q, k, per_file=m))
        ids = got[1][-1].astype(np.int64)  # the planted query: its row and the copy lead, the lower id first
        assert ids[1] == ids[0] + half and got[0][-1][0] == got[0][-1][1]
    sh.close(); single.close()


# ---- 5. scoped -------------------------------------------------------------------------------------------------------------

def test_sharded_grouped_scoped(VS):
    n, dim, k = 3000, 384, 10
    rows = synth_rows(7600, 0, n, dim)
    single, sh = _pair(VS, rows, 4, 100)
    other = VS(None, dim, devices=[0] * 4, rows_per_stripe=100)
    other.insert_embeddings(rows[:500])
    other.build_index()
    _set((single, sh), np.arange(n), _layout("files", n, 6))
    q = _queries(rows, 7601, 3)
    tenth = np.flatnonzero(np.random.default_rng(7).random(n) < 0.1)
    for name, ids in (("all", np.arange(n)), ("tenth", tenth), ("one stripe", np.arange(100, 200)), ("empty", np.array([], np.int64))):
        s1, s4 = single.scope(ids), sh.scope(ids)
        before = s4.route_info()[1]
        sh.search_raw(q, k, per_file=1)  # unscoped first: every shard's slot of the pooled context holds keys
        for m in (1, 3):
            _same(sh.search_raw(q, k, scope=s4, per_file=m), single.search_raw(q, k, scope=s1, per_file=m))
        live_parts = len({int(i) // 100 % 4 for i in ids})
        assert s4.route_info()[1] - before == 2 * live_parts, name  # a gathered search per shard part that holds a row
        if name == "one stripe":  # ids [100, 200) are shard 1's: the other three slots came back empty, not stale
            got = sh.search_raw(q, 200, scope=s4, per_file=3)
            assert ((got[1] >= 100) & (got[1] < 200) | (got[1] == 0xFFFFFFFF)).all() and got[2].max() <= 100
            _same(got, single.search_raw(q, 200, scope=s1, per_file=3))
        if name == "empty":
            got = sh.search_raw(q, k, scope=s4, per_file=1)
            assert got[2].tolist() == [0, 0, 0] and (got[1] == 0xFFFFFFFF).all()
        s1.close(); s4.close()
    foreign = other.scope(np.arange(100))
    with pytest.raises(_lib.CsError, match="the scope was made for another store") as e:
        sh.search_raw(q, k, scope=foreign, per_file=1)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    foreign.close()
    other.close(); sh.close(); single.close()


# ---- 6. variants -----------------------------------------------------------------------------------------------------------

def test_sharded_grouped_variants(VS):
    """Nine variants, and 16 at k = 1,000 (two levels of the capped variants merge), with and without a scope; the hog spread
    over the shards AND over the variants."""
    n, dim = 4000, 384
    rows = synth_rows(7700, 0, n, dim)
    center = synth_rows(7701, 0, 1, dim)[0]
    rows[:600] = center + 0.02 * rows[:600]
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    groups[:600] = 0
    single, sh = _pair(VS, rows, 4, 7)
    _set((single, sh), np.arange(n), groups)
    scope_ids = np.flatnonzero(np.arange(n) % 3 != 1)
    s1, s4 = single.scope(scope_ids), sh.scope(scope_ids)
    for nv, k in ((9, 10), (9, 200), (16, 1000)):
        q = center + 0.05 * synth_rows(7702 + nv, 0, nv, dim)  # every variant's plain top-k is the hog's
        for m in (1, 3):
            got = sh.search_variants_raw(q, k, per_file=m)
            _same(got, single.search_variants_raw(q, k, per_file=m))
            assert (groups[got[1][:got[2]]] == 0).sum() == m and got[2] == min(k, m * (1 + (n - 600) // 8))
            _same(sh.search_variants_raw(q, k, scope=s4, per_file=m), single.search_variants_raw(q, k, scope=s1, per_file=m))
    s1.close(); s4.close()
    sh.close(); single.close()


# ---- 7. the two equalities --------------------------------------------------------------------------------------------------

def test_uncapped_equals_the_plain_sharded_searches(VS):
    n, dim, k = 2500, 384, 20
    rows = synth_rows(7800, 0, n, dim)
    single, sh = _pair(VS, rows, 3, 50)
    single.close()
    q = _queries(rows, 7801, 9)
    sc = sh.scope(np.arange(0, n, 2))

    def check(m):
        _same(sh.search_raw(q, k, per_file=m), sh.search_raw(q, k))
        _same(sh.search_raw(q, k, scope=sc, per_file=m), sh.search_raw(q, k, scope=sc))
        _same(sh.search_variants_raw(q, k, per_file=m), sh.search_variants_raw(q, k))
        _same(sh.search_variants_raw(q, k, scope=sc, per_file=m), sh.search_variants_raw(q, k, scope=sc))

    assert sh.groups_info() == (0, 0)
    check(1)  # no group assigned: nothing is capped, and no table is made
    assert sh.groups_info() == (0, 0)
    sh.set_groups(np.arange(n), np.arange(n) % 5)
    check(k)  # per_group >= k
    check(k + 7)
    with pytest.raises(AssertionError):
        check(1)  # (and the cap does change the answer of this corpus)
    assert sh.groups_info()[1] >= 8 * n  # 4 B per id on the root and 4 B on its shard
    sc.close()
    sh.close()


# ---- 8. life cycle ----------------------------------------------------------------------------------------------------------

def test_groups_follow_the_sharded_store_life_cycle(VS):
    n, dim, k = 2000, 384, 30
    rows = synth_rows(7900, 0, n + 500, dim)
    single, sh = _pair(VS, rows[:n], 4, 7)
    stores = (single, sh)
    q = _queries(rows, 7901, 4)

    def check(m=2):
        got = sh.search_raw(q, k, per_file=m)
        _same(got, single.search_raw(q, k, per_file=m))
        assert sh.groups_info()[0] == single.groups_info()[0]
        return got

    _set(stores, np.arange(n), np.arange(n) // 8)
    check()
    dead = np.flatnonzero(np.random.default_rng(8).random(n) < 0.4)
    for st in stores:
        assert st.delete_chunks(dead) == len(dead)
        st.build_index()  # every shard reclaims its own deleted rows; the groups stay with the ids
    assert sh.stored_rows() == n - len(dead)
    check()
    for st in stores:
        assert st.insert_embeddings(rows[n:]).tolist() == list(range(n, n + 500))
        st.build_index()
    got = check(1)  # the new ids carry no group: any number of them may answer
    _set(stores, np.arange(n, n + 500), np.full(500, 4_000_000))
    capped = check(1)
    assert got[2].tolist() == capped[2].tolist() == [k] * len(q)  # (no empty slot, whose id would read as a large one)
    assert (capped[1] >= n).sum(axis=1).max() <= 1 and (got[1] >= n).sum() >= (capped[1] >= n).sum()
    # an id at or above next_id: refused, and nothing is assigned on any shard
    before = [sh.search_raw(q, k, per_file=1), sh.groups_info()]
    with pytest.raises(_lib.CsError, match=r"ids\[3\] = %d was never issued \(the index has issued ids 0 to %d\)" % (n + 500, n + 500)) as e:
        sh.set_groups([0, 1, 2, n + 500], [9, 9, 9, 9])
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    with pytest.raises(_lib.CsError, match="was never issued"):
        single.set_groups([0, 1, 2, n + 500], [9, 9, 9, 9])
    _same(sh.search_raw(q, k, per_file=1), before[0])
    assert sh.groups_info() == before[1]
    check(1)
    for st in stores:
        st.clear()
        assert st.groups_info()[0] == 0
        st.insert_embeddings(rows[:n])
        st.build_index()
    _same(check(1), sh.search_raw(q, k))  # nothing is grouped after clear()
    sh.close(); single.close()


# ---- 9. errors ---------------------------------------------------------------------------------------------------------------

def _raw_call(lib, name, h, scope, q, nq, dim, k, m):
    """One C call of either family -> (status, message)."""
    cos, ids = np.zeros(max(nq * k, 1), np.float32), np.zeros(max(nq * k, 1), np.uint32)
    cnt, flag = np.zeros(max(nq, 1), np.uint32), C.c_int32()
    args = [h] + ([scope] if "scoped" in name else []) + [q.ctypes.data_as(f32p), nq, dim, k, m, cos.ctypes.data_as(f32p),
                                                          ids.ctypes.data_as(u32p), cnt.ctypes.data_as(u32p)]
    if "variants" in name:
        args.append(C.byref(flag))
    st = getattr(lib, name)(*args)
    return st, (lib.cs_last_error().decode() if st else "")


def test_errors_their_texts_and_order(VS, gpu_lib):
    n, dim = 300, 384
    rows = synth_rows(8000, 0, n, dim)
    single, sh = _pair(VS, rows, 3, 10)
    unbuilt1, unbuilt3 = VS(None, dim), VS(None, dim, devices=[0] * 3, rows_per_stripe=10)
    unbuilt1.insert_embeddings(rows); unbuilt3.insert_embeddings(rows)
    other1, other3 = VS(None, dim), VS(None, dim, devices=[0] * 3, rows_per_stripe=10)
    s1, s3 = single.scope(np.arange(n)), sh.scope(np.arange(n))
    f1, f3 = other1.scope([1, 2]), other3.scope([1, 2])
    q = synth_rows(8001, 0, 20, dim)
    for kind in ("search_grouped", "search_grouped_scoped", "search_variants_grouped", "search_variants_grouped_scoped"):
        def both(st1, st3, sc1, sc3, nq, d, k, m):
            h = [None if x is None else x.handle for x in (st1, st3, sc1, sc3)]
            return (_raw_call(gpu_lib, "cs_index_" + kind, h[0], h[2], q, nq, d, k, m),
                    _raw_call(gpu_lib, "cs_shards_" + kind, h[1], h[3], q, nq, d, k, m))

        a, b = both(None, None, s1, s3, 1, dim, 5, 1)  # a null handle, before everything else (dim, nq and k are fine here)
        assert a[0] == b[0] == _lib.CS_ERR_BAD_ARG and a[1] == "null index handle" and b[1] == "null shards handle"
        cases = [(single, sh, s1, s3, 1, dim + 1, 0, 0),        # the dimension, before k, per_group and the scope
                 (unbuilt1, unbuilt3, None, None, 0, dim, 0, 0),  # not built, before nq
                 (single, sh, None, None, 0, dim, 0, 0),          # nq, before k
                 (single, sh, None, None, _lib.CS_MAX_QUERIES + 1, dim, 5, 1),
                 (single, sh, None, None, 1, dim, 0, 0),          # k, before per_group
                 (single, sh, None, None, 1, dim, _lib.CS_MAX_K + 1, 0),
                 (single, sh, None, None, 1, dim, 5, 0)]          # per_group, before the scope's
        if "variants" in kind:
            cases.append((single, sh, None, None, 17, dim, 5, 0))  # the variants limit, before per_group
        if "scoped" in kind:
            cases += [(single, sh, None, None, 1, dim, 5, 1),     # a null scope
                      (single, sh, f1, f3, 1, dim, 5, 1)]         # a scope of another store
        for case in cases:
            a, b = both(*case)
            assert a[0] != _lib.CS_OK and a == b, (kind, case[4:], a, b)
        a, b = both(single, sh, s1, s3, 2, dim, 5, 1)
        assert a == b == (_lib.CS_OK, "")
    for st in (s1, s3, f1, f3, unbuilt1, unbuilt3, other1, other3, single, sh):
        st.close()


# ---- 10. direct gather -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("direct", ["1", "0"])
def test_gather_modes(VS, monkeypatch, direct):
    monkeypatch.setenv("CS_SHARDS_DIRECT", direct)
    n, dim = 2003, 384
    rows = synth_rows(7100 + dim, 0, n, dim)
    single, sh = _pair(VS, rows, 4, 7)
    assert bool(sh._lib.cs_shards_direct_gather(sh.handle)) == (direct == "1")
    _set((single, sh), np.arange(n), _layout("files", n, 5))
    sc1, sc4 = single.scope(np.arange(100, 200)), sh.scope(np.arange(100, 200))
    for nq in (1, 9):
        q = _queries(rows, 7200 + nq, nq)
        for k in (10, 200):
            _same(sh.search_raw(q, k, per_file=1), single.search_raw(q, k, per_file=1))
            _same(sh.search_raw(q, k, scope=sc4, per_file=1), single.search_raw(q, k, scope=sc1, per_file=1))
            _same(sh.search_variants_raw(q, k, per_file=3), single.search_variants_raw(q, k, per_file=3))
    sc1.close(); sc4.close()
    sh.close(); single.close()


# ---- 11. concurrent searches ---------------------------------------------------------------------------------------------------

def test_concurrent_sharded_grouped_searches(VS):
    n, dim, k = 4000, 384, 25
    rows = synth_rows(8100, 0, n, dim)
    single, sh = _pair(VS, rows, 4, 7)
    single.close()
    sh.set_groups(np.arange(n), np.arange(n) % 9)
    q = _queries(rows, 8101, 2)
    caps = [1, 2, 3, 5]
    want = [sh.search_raw(q, k, per_file=m) for m in caps]
    assert len({w[1].tobytes() for w in want}) == len(caps)  # four different answers
    errors = []

    def work(t):
        try:
            for _ in range(20):
                _same(sh.search_raw(q, k, per_file=caps[t]), want[t])
        except BaseException as e:  # noqa: BLE001 — reported by the main thread
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
    sh.close()


# ---- 12. the Python surface ----------------------------------------------------------------------------------------------------

def test_per_file_on_the_python_surface_of_a_sharded_store(VS):
    from codesearch_amd import Chunk, EmbeddedChunk

    n, dim = 240, 384
    rows = synth_rows(8200, 0, n, dim)
    q = synth_rows(8201, 0, 3, dim)
    rows[:40] = q[0] + 0.02 * rows[:40]
    paths = ["hog.rs" if i < 40 else "f%d.rs" % (i // 6) for i in range(n)]
    chunks = [EmbeddedChunk(Chunk("fn c%d() {}" % i, i, i + 1, "Function", paths[i]), rows[i].tolist()) for i in range(n)]
    single, sh = VS(None, dim), VS(None, dim, devices=[0, 0, 0], rows_per_stripe=4, grouped=True)
    for st in (single, sh):
        assert st.insert_chunks_with_ids(chunks) == list(range(n))
        st.build_index()
    assert sh.groups_info()[0] == single.groups_info()[0] == n  # a chunk's file is its group on a sharded store too
    ids = np.arange(0, n, 2)
    s1, s3 = single.scope(ids), sh.scope(ids)
    got = sh.search(q[0], 8, per_file=1)
    assert got == single.search(q[0], 8, per_file=1) and len({r.path for r in got}) == 8 and got[0].path == "hog.rs"
    assert sh.search(q[0], 8, scope=s3, per_file=2) == single.search(q[0], 8, scope=s1, per_file=2)
    assert sh.search_batch(q, 8, per_file=1) == single.search_batch(q, 8, per_file=1)
    assert sh.search_batch(q, 8, scope=s3, per_file=1) == single.search_batch(q, 8, scope=s1, per_file=1)
    assert sh.search_variants(q, 8, per_file=1) == single.search_variants(q, 8, per_file=1)
    assert sh.search_variants(q, 8, scope=s3, per_file=2) == single.search_variants(q, 8, scope=s1, per_file=2)
    for call in (lambda: sh.search_variants_raw(q, 8, per_file=1, class_weights=[1.0, 2.0]),
                 lambda: sh.search_variants(q, 8, per_file=1, boost_kind="Function")):
        with pytest.raises(_lib.CsError, match="a sharded store has no boosted search") as e:
            call()
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="exclusive"):  # a bitmap mask with per_file=: refused as on a single store
        sh.search_raw(q, 8, chunk_ids=[1, 2, 3], per_file=1)
    s1.close(); s3.close()
    sh.close(); single.close()


# ---- 13. the C++ mirror --------------------------------------------------------------------------------------------------------

def test_cpp_host_mirror_sharded_per_file(gpu_lib):
    """host/codesearch_gpu.hpp: set_groups, search_per_file and search_variants_per_file of a sharded VectorStore
    (tests/cpp/shards_grouped_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "shards_grouped_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "shards_grouped_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "shards grouped host ok" in r.stdout


# ---- 14. the opt-in ---------------------------------------------------------------------------------------------------------------

def test_a_sharded_store_opened_without_grouped_refuses_as_before(VS):
    sh = VS(None, 384, devices=[0, 0])
    for call in (lambda: sh.groups_info(), lambda: sh.set_groups([0], [0]),
                 lambda: sh.search_raw(np.zeros(384, np.float32), 5, per_file=1),
                 lambda: sh.search_variants_raw(np.zeros((2, 384), np.float32), 5, per_file=1)):
        with pytest.raises(_lib.CsError, match="sharded store has no grouped search.*grouped=True") as e:
            call()
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    sh.close()
