"""Similar-chunk search (cs_index_search_similar, codesearch_amd/csrc/scan_similar.hip): the exact best k stored chunks for
a query that is itself a stored chunk, without the chunk — or the chunk's whole file — decided inside the selection.

Ground truth comes only from code that exists without the feature: the source's row read back (read_rows), the full
(cosine desc, id asc) order of the store for it — search_raw(row, n) on the streaming route for up to 1,024 live rows (with
its cosine bits), the CPU oracle above that — reduced on the host by search.drop_excluded.  Ids and counts must match
exactly; cosines bit for bit wherever the streaming search returns the id, else within the suite's 1e-4 of the oracle."""
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, drop_excluded
from codesearch_amd.synth import synth_rows
from codesearch_amd.vector_store import cos_to_score

pytestmark = pytest.mark.gpu

MODES = ("none", "self", "file")


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


def _full_order(st, q):
    """(cos, ids) of every live row of a store of at most 1,024 live rows, (cosine desc, id asc): one streaming search."""
    n = len(st)
    assert 0 < n <= 1024
    c, i, cnt = st.search_raw(q, n)
    assert cnt[0] == n
    return c[0].copy(), i[0].copy()


def _truth(st, srcs):
    """{source id: full order of the store for that source's stored row}, one streaming search per distinct source."""
    return {int(s): _full_order(st, st.read_rows(int(s) - st.id_base, 1)[0]) for s in set(int(x) for x in srcs)}


def _group_lookup(groups: dict):
    return lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]


def _check(st, truth, lookup, srcs, k, mode, min_cos=None):
    """st.similar_raw(srcs, k, mode, min_cos) against truth[source] reduced on the host; -> the counts."""
    cos, ids, cnt = st.similar_raw(srcs, k, exclude=mode, min_cos=min_cos)
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


SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1000, 1), (10, 40)]  # (k, nq): query tiles 1, 2 and 4 and a ragged last tile


def _files_of_8(n, ungrouped):
    """ids in files of 8 consecutive ids; the last `ungrouped` ids carry no group."""
    return {r: r // 8 for r in range(n - ungrouped)}


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_similar_equals_reduced_full_order(VS, dim):
    n, seed = 1000, 9500 + dim
    rows = synth_rows(seed, 0, n, dim)
    st = _store(VS, rows)
    # one query tile of four holds two sources of one file (16, 17), one of another (100) and an ungrouped one (970); the
    # same source comes twice in one call (16, then 970 and 100 again further on)
    srcs = [16, 17, 100, 970, 16, 23, 999, 0, 7, 8, 960, 959, 500, 501, 502, 503, 970, 100]
    srcs += [int(x) for x in np.random.default_rng(seed).integers(0, n, 40 - len(srcs))]
    truth = _truth(st, srcs)
    assert all(truth[s][1][0] == s for s in truth)  # synthetic rows are distinct: a row is its own nearest
    # no group assigned: "file" is "self"
    for k, nq in SHAPES:
        a, b = st.similar_raw(srcs[:nq], k, exclude="file"), st.similar_raw(srcs[:nq], k, exclude="self")
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    for mode in MODES:
        for k, nq in SHAPES:
            cnt = _check(st, truth, look, srcs[:nq], k, mode)
            if k == 1000:
                assert cnt[0] == {"none": 1000, "self": 999, "file": 992}[mode]
    # a source's own answer does not depend on its neighbours in the call
    alone = st.similar_raw([970], 10, exclude="file")
    batch = st.similar_raw(srcs[:9], 10, exclude="file")
    assert all(x[0].tobytes() == y[3].tobytes() for x, y in zip(alone, batch))
    st.close()


@pytest.mark.parametrize("k", [1, 10, 200])
def test_exclude_none_is_the_streaming_search_of_the_row(VS, k):
    n, dim = 3000, 384
    rows = synth_rows(9601, 0, n, dim)
    rows[5] = rows[700]  # an identical row with a lower id: it wins the tie
    st = _store(VS, rows)
    srcs = [700, 5, 123, 2999]
    cos, ids, cnt = st.similar_raw(srcs, k, exclude="none")
    for q, s in enumerate(srcs):
        want = st.search_raw(st.read_rows(s, 1)[0], k)
        assert cnt[q] == want[2][0] == k
        assert ids[q].tobytes() == want[1][0].tobytes() and cos[q].tobytes() == want[0][0].tobytes()
    assert ids[0][0] == 5 and ids[1][0] == 5 and ids[2][0] == 123 and ids[3][0] == 2999
    if k > 1:
        assert ids[0][1] == 700 and cos[0][0].tobytes() == cos[0][1].tobytes()
    st.close()


def test_a_file_of_near_duplicates_does_not_crowd_out_the_rest(VS):
    """600 rows of the source's file are 0.95 s + 0.05 noise.  Excluding the file inside the selection returns ten chunks of
    other files; what a caller can do without it — search with the row, drop the file from the ranked list — finds none."""
    n, dim, k = 1000, 384, 10
    rows = synth_rows(9701, 0, n, dim)
    hog = np.arange(200, 800)
    src = 200
    rows[hog[1:]] = 0.95 * rows[src] + 0.05 * rows[hog[1:]]
    groups = {r: 1000 + r // 8 for r in range(n)}
    groups.update({int(r): 7 for r in hog})
    st = _store(VS, rows)
    st.set_groups(list(groups), list(groups.values()))
    truth = _truth(st, [src, 201, 0])
    look = _group_lookup(groups)
    cnt = _check(st, truth, look, [src], k, "file")
    assert cnt[0] == k
    got = st.similar_raw([src], k, exclude="file")[1][0].tolist()
    assert all(groups[i] != 7 for i in got)
    c, i, c_n = st.search_raw(st.read_rows(src, 1)[0], 200)
    post = [x for x in i[0][:c_n[0]].tolist() if groups[x] != 7]
    assert len(post) < k  # the rank-then-filter a caller is left with today
    _check(st, truth, look, [src, 201, 0], k, "self")
    _check(st, truth, look, [src, 201, 0], 200, "file")
    st.close()


def test_min_cos_is_a_strict_bound(VS):
    n, dim = 1000, 384
    rows = synth_rows(9801, 0, n, dim)
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    srcs = [50, 51, 975]
    truth = _truth(st, srcs)
    for mode in MODES:
        kept_c, _ = drop_excluded(*truth[50], look(truth[50][1]), 50, groups[50], mode, None, 20)
        fifth = np.float32(kept_c[4])
        assert kept_c[3] > fifth  # (distinct cosines: the bound cuts between the 4th and the 5th)
        cnt = _check(st, truth, look, [50], 20, mode, min_cos=fifth)
        assert cnt[0] == 4  # strict: the 5th hit itself is not above its own cosine
        for k, m in [(10, float(fifth)), (200, 0.0), (1000, -0.02), (10, 0.05)]:
            _check(st, truth, look, srcs, k, mode, min_cos=np.float32(m))
        cos, ids, cnt = st.similar_raw(srcs, 10, exclude=mode, min_cos=2.0)  # above every cosine
        assert (cnt == 0).all() and (ids == 0xFFFFFFFF).all() and (cos == 0).all()
        a, b = st.similar_raw(srcs, 10, exclude=mode, min_cos=float("-inf")), st.similar_raw(srcs, 10, exclude=mode)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        with pytest.raises(_lib.CsError, match="min_cos is NaN"):
            st.similar_raw(srcs, 10, exclude=mode, min_cos=float("nan"))
    st.close()


@pytest.mark.parametrize("dim", [384, 100])
def test_small_stores(VS, dim):
    one = _store(VS, synth_rows(9901, 0, 1, dim))
    cos, ids, cnt = one.similar_raw([0], 5, exclude="self")
    assert cnt[0] == 0 and (ids == 0xFFFFFFFF).all() and (cos == 0).all()
    cos, ids, cnt = one.similar_raw([0], 5, exclude="none")
    want = one.search_raw(one.read_rows(0, 1)[0], 5)
    assert cnt[0] == 1 and ids[0][0] == 0 and cos.tobytes() == want[0].tobytes() and ids.tobytes() == want[1].tobytes()
    one.close()

    st = _store(VS, synth_rows(9902, 0, 17, dim))
    truth = _truth(st, range(17))
    groups = {r: r // 8 for r in range(16)}
    st.set_groups(list(groups), list(groups.values()))
    for mode in MODES:
        cnt = _check(st, truth, _group_lookup(groups), list(range(17)), 200, mode)
        assert cnt.tolist() == {"none": [17] * 17, "self": [16] * 17, "file": [9] * 16 + [16]}[mode]
    everyone = {r: 4 for r in range(17)}  # every row in the source's file
    st.set_groups(list(everyone), list(everyone.values()))
    cnt = _check(st, truth, _group_lookup(everyone), [3, 16], 200, "file")
    assert cnt.tolist() == [0, 0]
    st.close()


def test_similar_follows_the_store_life_cycle(VS):
    n, dim, base, k = 900, 384, 5000, 10
    rows = synth_rows(9911, 0, n, dim)
    st = _store(VS, rows, id_base=base)
    groups = {base + r: r // 8 for r in range(n)}
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)
    src, victim = base + 101, base + 333
    srcs = [src, base + 102, base + 899, base]
    truth = _truth(st, srcs)

    def check_all(t):
        for mode in MODES:
            for kk in (k, 200):
                _check(st, t, look, srcs, kk, mode)

    check_all(truth)
    # a few deletes, among them the source's nearest neighbours: the build does not reclaim yet, the rows are tombstones
    near = [int(i) for i in truth[src][1][1:] if int(i) not in srcs and int(i) != victim][:3]
    first = sorted(set(near + [victim] + [base + r for r in range(7, n, 40)]) - set(srcs))
    assert st.delete_chunks(first) == len(first) and len(first) * 10 < n
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.similar_raw(srcs, k)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.stored_rows() == n and len(st) == n - len(first)
    truth = _truth(st, srcs)
    check_all(truth)
    got = st.similar_raw([src], k, exclude="self")[1][0].tolist()
    assert not set(got) & set(near)
    with pytest.raises(_lib.CsError, match=r"ids\[1\] = %d: the chunk was deleted" % victim) as e:
        st.similar_raw([src, victim], k)
    assert e.value.code == _lib.CS_ERR_BAD_ARG
    # 30 % deleted in all: the build reclaims, rows move, ids and groups stay
    pool = [base + r for r in range(n) if base + r not in srcs and base + r not in first]
    more = sorted(pool, key=lambda i: ((i - base) % 10 not in (0, 3, 7), i))[:(3 * n) // 10 - len(first)]
    assert st.delete_chunks(more) == len(more)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    gone = set(first) | set(more)
    assert len(gone) == (3 * n) // 10 and st.stored_rows() == len(st) == n - len(gone)
    truth = _truth(st, srcs)
    check_all(truth)
    # ... and the answers are those of a fresh store of the survivors, mapped through their ids, bit for bit
    alive = np.array([base + r for r in range(n) if base + r not in gone])
    fresh = _store(VS, rows[alive - base])
    fresh.set_groups(np.arange(len(alive)), [groups[int(i)] for i in alive])
    where = {int(i): j for j, i in enumerate(alive)}
    for mode in MODES:
        a = st.similar_raw(srcs, 200, exclude=mode)
        b = fresh.similar_raw([where[s] for s in srcs], 200, exclude=mode)
        assert a[0].tobytes() == b[0].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert a[1].tolist() == [[int(alive[j]) if j != 0xFFFFFFFF else j for j in row] for row in b[1].tolist()]
    fresh.close()
    # a deleted source is refused after the reclaim as before it; an id never issued is refused, below and above
    for bad, text in [(victim, "the chunk was deleted"), (more[0], "the chunk was deleted"), (base - 1, "never issued"),
                      (st.next_id(), "never issued"), (0, "never issued")]:
        with pytest.raises(_lib.CsError, match=text) as e:
            st.similar_raw([src, src, bad], k)
        assert e.value.code == _lib.CS_ERR_BAD_ARG and "ids[2] = %d" % bad in str(e.value)
    # appended rows are found (they carry no group: "file" keeps them); an assignment needs no build
    s_row = st.read_rows(src - base, 1)[0]
    new = st.insert_embeddings(np.stack([0.95 * s_row + 0.05 * rows[j] for j in range(6)])).tolist()
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    truth = _truth(st, srcs + new[:1])
    check_all(truth)
    for mode in ("self", "file"):
        assert sorted(st.similar_raw([src], 6, exclude=mode)[1][0].tolist()) == sorted(new)
    _check(st, truth, look, [new[0], src], k, "file")
    for i in new:
        groups[i] = groups[src]
    st.set_groups(new, [groups[src]] * len(new))
    assert not set(st.similar_raw([src], k, exclude="file")[1][0].tolist()) & set(new)
    assert sorted(st.similar_raw([src], 6, exclude="self")[1][0].tolist()) == sorted(new)
    check_all(truth)
    # clear(): no id is issued any more
    st.clear()
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.similar_raw([src], k)
    st.build_index()
    for i in (src, base, new[0]):
        with pytest.raises(_lib.CsError, match="never issued"):
            st.similar_raw([i], k)
    st.close()


def _same_bits_as_the_stream(st, q, cos, ids, stream_depth=1024):
    """An answer's cosines against the streaming search's, bit for bit, for every id that search returns among its
    `stream_depth` best; -> how many ids were compared."""
    sc, si, sn = st.search_raw(q, min(stream_depth, len(st)))
    bits = dict(zip(si[0][:sn[0]].tolist(), sc[0][:sn[0]]))
    seen = 0
    for c, i in zip(cos, ids.tolist()):
        if i in bits:
            assert np.float32(c).tobytes() == np.float32(bits[i]).tobytes(), i
            seen += 1
    return seen


def test_many_blocks_and_a_merge_level_against_the_oracle(VS, oracle):
    n, dim, k, hog = 20_000, 384, 200, 3000
    rows = synth_rows(9921, 0, n, dim)
    hog_rows = np.arange(6000, 6000 + hog)
    rows[hog_rows[1:]] = 0.9 * rows[hog_rows[0]] + 0.1 * rows[hog_rows[1:]]
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    groups[hog_rows] = 0
    groups[n - 40:] = NO_GROUP
    st = _store(VS, rows)
    st.set_groups(np.arange(n), groups)
    srcs = [6000, 6001, 40, n - 1, 8999]  # two sources inside the file, its last row, a small file, an ungrouped row
    cos, ids, cnt = st.similar_raw(srcs, k, exclude="file")
    for q, s in enumerate(srcs):
        oc, oi = oracle.scan_topk(rows, rows[s], n, mode="omp")
        ec, ei = drop_excluded(oc, oi, groups[oi], s, int(groups[s]), "file", None, k)
        assert len(ei) == k and cnt[q] == k
        assert ids[q].tolist() == ei, (q, s)
        assert np.abs(cos[q] - np.asarray(ec, np.float32)).max() < 1e-4
        assert not (groups[ids[q]] == groups[s]).any() or groups[s] == NO_GROUP
        seen = _same_bits_as_the_stream(st, st.read_rows(s, 1)[0], cos[q], ids[q])
        assert seen == k or groups[s] == 0  # (a source in the file: the stream's 1,024 best are the file's rows)
        one = st.similar_raw([s], k, exclude="file")  # one source per call: the single-query launch, the same levels
        assert one[2][0] == k and one[1][0].tobytes() == ids[q].tobytes() and one[0][0].tobytes() == cos[q].tobytes()
    st.close()


def _raw_call(lib, h, ids, nq, k, exclude, min_cos, cos, out_ids, counts):
    p = lambda a, t: a.ctypes.data_as(t) if a is not None else None
    return lib.cs_index_search_similar(h, p(ids, _lib.u32p), nq, k, exclude, min_cos, p(cos, _lib.f32p), p(out_ids, _lib.u32p),
                                       p(counts, _lib.u32p))


def test_errors_and_their_order(VS, gpu_lib):
    n, dim, k = 500, 384, 5
    st = VS(None, dim, id_base=100)
    st.insert_embeddings(synth_rows(9931, 0, n, dim))
    src = np.array([100, 101], np.uint32)
    cos = np.full((2, k), 7.0, np.float32)
    ids = np.full((2, k), 7, np.uint32)
    counts = np.full(2, 7, np.uint32)
    nan, inf = float("nan"), float("-inf")

    def fails(text, *a, handle=True):
        assert _raw_call(gpu_lib, st.handle if handle else None, *a) == _lib.CS_ERR_BAD_ARG
        assert text in _lib.last_error(), _lib.last_error()
        assert (cos == 7.0).all() and (ids == 7).all() and (counts == 7).all()  # a failing call writes nothing

    # 1. cs_index_search's own, in its order: the handle, the build, nq, k — each before everything behind it
    fails("null index handle", None, 0, 0, 9, nan, None, None, None, handle=False)
    assert _raw_call(gpu_lib, st.handle, None, 0, 0, 9, nan, None, None, None) == _lib.CS_ERR_NOT_BUILT
    assert "Index not built. Call build_index() after inserting chunks." in _lib.last_error()
    st.build_index()
    fails("nq must be in 1..4096, got 0", None, 0, 0, 9, nan, None, None, None)
    fails("nq must be in 1..4096, got 4097", None, 4097, 0, 9, nan, None, None, None)
    fails("k must be in 1..1024, got 0", None, 2, 0, 9, nan, None, None, None)
    fails("k must be in 1..1024, got 1025", None, 2, 1025, 9, nan, None, None, None)
    # 2. null buffers, before the mode
    fails("null buffer", None, 2, k, 9, nan, cos, ids, counts)
    fails("null buffer", src, 2, k, 9, nan, None, ids, counts)
    fails("null buffer", src, 2, k, 9, nan, cos, None, counts)
    fails("null buffer", src, 2, k, 9, nan, cos, ids, None)
    # 3. the mode, before the bound;  4. the bound, before the ids
    bad = np.array([100, 99], np.uint32)
    fails("exclude must be", src, 2, k, 3, nan, cos, ids, counts)
    fails("exclude must be", src, 2, k, -1, nan, cos, ids, counts)
    fails("min_cos is NaN", bad, 2, k, 2, nan, cos, ids, counts)
    # 5. the ids: the first offending one is named
    fails("ids[1] = 99 was never issued", bad, 2, k, 2, inf, cos, ids, counts)
    fails("ids[0] = 600 was never issued", np.array([600, 99], np.uint32), 2, k, 0, 0.5, cos, ids, counts)
    assert st.delete_chunks([150]) == 1
    st.build_index()
    fails("ids[1] = 150: the chunk was deleted", np.array([100, 150, 99], np.uint32), 3, k, 1, inf, cos, ids, counts)
    fails("ids[0] = 99 was never issued", np.array([99, 150], np.uint32), 2, k, 1, inf, cos, ids, counts)
    assert _raw_call(gpu_lib, st.handle, src, 2, k, 1, inf, cos, ids, counts) == _lib.CS_OK
    assert counts.tolist() == [k, k] and (ids != 7).all()
    # the Python layer's own checks
    with pytest.raises(ValueError, match="exclude must be"):
        st.similar_raw([100], k, exclude="group")
    with pytest.raises(_lib.CsError, match="nq must be in 1..4096, got 0"):
        st.similar_raw([], k)
    st.close()


def test_concurrent_similar_searches(VS):
    n, dim, k = 60_000, 384, 25
    st = VS(None, dim)
    st.insert_synthetic(n, 0xC0C4, 0)
    st.build_index()
    st.set_groups(np.arange(n), np.arange(n) // 8)
    rng = np.random.default_rng(11)
    jobs = [(rng.integers(0, n, nq).tolist(), mode, bound) for nq, mode, bound in
            [(1, "self", None), (3, "file", None), (9, "none", 0.0), (2, "file", 0.05)]]
    before = st.search_raw(synth_rows(0xC0C5, 0, 2, dim), k)
    want = [st.similar_raw(s, k, exclude=m, min_cos=b) for s, m, b in jobs]
    assert all(int(w[2].max()) > 0 for w in want)
    errors = []

    def work(t):
        try:
            s, m, b = jobs[t]
            for _ in range(20):
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
    after = st.search_raw(synth_rows(0xC0C5, 0, 2, dim), k)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_similar_returns_results_with_metadata(VS):
    dim, per = 384, 12
    files = ["vendor/gen.rs", "src/a.rs", "src/b.rs", "src/c.rs", "lib/d.rs"]
    noise = synth_rows(9941, 0, per * len(files), dim)
    paths = [files[i % len(files)] for i in range(len(noise))]  # the files' chunks interleaved: groups are not id ranges
    rows = noise.copy()
    hog = [i for i, p in enumerate(paths) if p == files[0]]
    src = hog[0]
    rows[hog[1:]] = 0.9 * rows[src] + 0.1 * noise[hog[1:]]  # one file of near-duplicates of its first chunk
    st = VS(None, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(len(paths)))
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    full_c, full_i = _full_order(st, st.read_rows(src, 1)[0])
    number = {}
    look = [number.setdefault(paths[int(i)], len(number)) for i in full_i]
    same = st.similar(src, 5)
    want = drop_excluded(full_c, full_i, look, src, number[files[0]], "self", None, 5)[1]
    assert [r.id for r in same] == want and {r.path for r in same} == {files[0]} and src not in want
    assert [r.content for r in same] == [f"chunk {i}" for i in want] and all(r.kind == "Function" for r in same)
    other = st.similar(src, 5, other_files=True)
    want_c, want_i = drop_excluded(full_c, full_i, look, src, number[files[0]], "file", None, 5)
    assert [r.id for r in other] == want_i and files[0] not in {r.path for r in other}
    assert [r.path for r in other] == [paths[i] for i in want_i]
    assert [np.float32(r.score) for r in other] == [cos_to_score(np.float32(c)) for c in want_c]
    assert other[0].score > other[-1].score
    # min_score is on the reference's score scale: a bound between the second and the third hit's scores keeps two
    assert same[1].score - same[2].score > 1e-5
    assert [r.id for r in st.similar(src, 5, min_score=(same[1].score + same[2].score) / 2)] == want[:2]
    assert st.similar(src, 5, min_score=1.0) == []
    st.close()
    sharded = VS(None, dim, devices=[0, 0])
    for call in (lambda: sharded.similar_raw([0], 5), lambda: sharded.similar(0, 5)):
        with pytest.raises(_lib.CsError, match="no similar-chunk search: no cs_shards_ form yet") as e:
            call()
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    with pytest.raises(_lib.CsError, match="sharded store has no grouped search"):  # the existing refusal keeps its text
        sharded.groups_info()
    sharded.close()


def test_more_sources_than_one_call_takes(VS):
    n, dim = 1000, 384
    st = _store(VS, synth_rows(9951, 0, n, dim))
    st.set_groups(np.arange(n), np.arange(n) // 8)
    srcs = np.arange(4100) % n
    for mode in ("self", "file"):
        once = st.similar_raw(np.arange(n), 1, exclude=mode)
        cos, ids, cnt = st.similar_raw(srcs, 1, exclude=mode)
        assert cos.shape == (4100, 1) and (cnt == 1).all()
        assert ids.tobytes() == once[1][srcs].tobytes() and cos.tobytes() == once[0][srcs].tobytes()
        assert (ids[:, 0] != srcs).all()
        if mode == "file":
            assert (ids[:, 0] // 8 != srcs // 8).all()
    truth = _truth(st, [0, 999, 4099 % n])
    _check(st, truth, lambda ids: [int(i) // 8 for i in ids], [0, 999, 4099 % n], 1, "file")
    st.close()


def test_cpp_wrapper_finds_similar_chunks():
    """host/codesearch_gpu.hpp: VectorStore::similar (tests/cpp/similar_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "similar_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "similar_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "similar host ok" in r.stdout
