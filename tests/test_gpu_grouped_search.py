"""Grouped search (cs_index_search_grouped, codesearch_amd/csrc/scan_grouped.hip): the exact best k rows with at most
per_group rows of one group — the exact form of the reference's `--per-file`, which caps each file's hits only after it
has ranked `max_results` of them (the reference's src/search/mod.rs:1007-1038).

Ground truth comes only from code that exists without the feature: the full (cosine desc, id asc) order of a store —
search_raw(q, n) on the streaming route for up to 1,024 live rows (with its cosine bits), the CPU oracle above that —
capped on the host by search.cap_per_group.  Ids must match exactly; cosines bit for bit wherever the streaming search
returns the same id, else within the suite's 1e-4 of the oracle."""
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, cap_per_group
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu


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


def _group_lookup(groups: dict):
    return lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]


def _check(st, truth, lookup, qs, k, m):
    """st.search_raw(qs, k, per_file=m) against truth[q] = the full order of query q, capped on the host."""
    cos, ids, cnt = st.search_raw(qs, k, per_file=m)
    for q in range(qs.shape[0]):
        tc, ti = truth[q]
        ec, ei = cap_per_group(tc, ti, lookup(ti), k, m)
        n = len(ei)
        assert cnt[q] == n, (q, k, m, cnt[q], n)
        assert ids[q][:n].tolist() == ei, (q, k, m)
        assert cos[q][:n].tobytes() == np.asarray(ec, np.float32).tobytes(), (q, k, m)
        assert (ids[q][n:] == 0xFFFFFFFF).all() and (cos[q][n:] == 0).all()


SHAPES = [(1, 1, 1), (10, 1, 1), (10, 3, 3), (200, 2, 9), (1000, 1, 1), (10, 1, 40)]  # (k, m, nq)


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_grouped_equals_capped_full_order(VS, dim):
    n, seed = 1000, 9100 + dim
    rows = synth_rows(seed, 0, n, dim)
    qs = np.concatenate([synth_rows(seed + 1, 0, 38, dim), rows[[5, n - 3]]])
    st = _store(VS, rows)
    truth = [_full_order(st, q) for q in qs]
    assert st.groups_info() == (0, 0)
    groupings = [
        ("none", {}),
        ("mod7", {r: r % 7 for r in range(n)}),
        ("files16", {r: r // 16 for r in range(n)}),
        ("one", {r: 3 for r in range(n)}),
    ]
    for name, groups in groupings:
        if groups:
            st.set_groups(list(groups), list(groups.values()))
            assert st.groups_info()[0] == n
        for k, m, nq in SHAPES:
            _check(st, truth, _group_lookup(groups), qs[:nq], k, m)
    st.close()


@pytest.mark.parametrize("dim", [384, 1024])
def test_long_lists_lower_the_query_tile(VS, dim):
    """Several queries with k above 256: 12 B per slot lowers the scan's query tile to two (kpad 512) and to one
    (kpad 1,024) queries per pass, so the launch makes several passes over blockIdx.y."""
    n, seed = 1000, 9300 + dim
    rows = synth_rows(seed, 0, n, dim)
    qs = synth_rows(seed + 1, 0, 5, dim)
    st = _store(VS, rows)
    truth = [_full_order(st, q) for q in qs]
    groups = {r: r // 16 for r in range(n)}
    st.set_groups(list(groups), list(groups.values()))
    for k, m, nq in [(300, 2, 3), (300, 5, 5), (1000, 2, 3), (1000, 16, 5)]:
        _check(st, truth, _group_lookup(groups), qs[:nq], k, m)
    st.close()


@pytest.mark.parametrize("k", [10, 200])
def test_uncapped_equals_the_streaming_search(VS, k):
    """per_group >= k, and no groups at all: cs_index_search on the streaming route, bit for bit."""
    n, dim = 5000, 384
    rows = synth_rows(77, 0, n, dim)
    qs = synth_rows(78, 0, 3, dim)
    st = _store(VS, rows)
    want = [st.search_raw(q, k) for q in qs]

    def same(got):
        for q in range(len(qs)):
            assert all(x[q].tobytes() == y[0].tobytes() for x, y in zip(got, want[q]))

    same(st.search_raw(qs, k, per_file=1))  # no groups assigned: nothing is capped
    st.set_groups(np.arange(n), np.arange(n) // 3)
    same(st.search_raw(qs, k, per_file=k))
    same(st.search_raw(qs, k, per_file=0xFFFFFFFF))
    st.set_groups(np.arange(n), np.full(n, NO_GROUP))  # un-assigned again
    assert st.groups_info()[0] == 0
    same(st.search_raw(qs, k, per_file=1))
    st.close()


def _same_bits_as_the_stream(st, q, cos, ids, stream_depth=1024):
    """A grouped answer's cosines against the streaming search's, bit for bit, for every id that search returns among its
    `stream_depth` best; -> how many ids were compared."""
    sc, si, sn = st.search_raw(q, min(stream_depth, len(st)))
    bits = dict(zip(si[0][:sn[0]].tolist(), sc[0][:sn[0]]))
    seen = 0
    for c, i in zip(cos, ids.tolist()):
        if i in bits:
            assert np.float32(c).tobytes() == np.float32(bits[i]).tobytes(), i
            seen += 1
    return seen


def _oracle_check(st, oracle, corpus, q, groups, k, m, depth, stream_depth=1024):
    """One query against the oracle's first `depth` rows, capped; -> the expected ids."""
    oc, oi = oracle.scan_topk(corpus, q, depth, mode="omp")
    ec, ei = cap_per_group(oc, oi, groups[oi], k, m)
    cos, ids, cnt = st.search_raw(q, k, per_file=m)
    assert cnt[0] == len(ei)
    assert ids[0][:cnt[0]].tolist() == ei
    assert np.abs(cos[0][:cnt[0]] - np.asarray(ec, np.float32)).max() < 1e-4
    _same_bits_as_the_stream(st, q, cos[0][:cnt[0]], ids[0][:cnt[0]], stream_depth)
    return ei


def test_fewer_groups_than_k(VS, oracle):
    """Five groups, k = 10, m = 1: five rows, and no list of the scan ever fills."""
    n, dim = 2000, 384
    rows = synth_rows(501, 0, n, dim)
    st = _store(VS, rows)
    groups = (np.arange(n) % 5).astype(np.uint32)
    st.set_groups(np.arange(n), groups)
    for q in synth_rows(502, 0, 2, dim):
        assert len(_oracle_check(st, oracle, rows, q, groups, 10, 1, n)) == 5
    st.close()


def test_one_file_of_near_duplicates_does_not_crowd_out_the_rest(VS, oracle):
    """3,000 rows of one group are 0.9 q + 0.1 noise.  k = 10, m = 1 holds one of them and nine others; capping the
    1,024 best rows on the host (CS_MAX_K: the most a post-cap can fetch) finds fewer than ten."""
    n, dim, hog = 12_000, 384, 3000
    rows = synth_rows(601, 0, n, dim)
    q = synth_rows(602, 0, 1, dim)[0]
    hog_rows = np.arange(4000, 4000 + hog)
    rows[hog_rows] = 0.9 * q + 0.1 * rows[hog_rows]
    groups = (np.arange(n) // 8 + 1).astype(np.uint32)
    groups[hog_rows] = 0
    st = _store(VS, rows)
    st.set_groups(np.arange(n), groups)
    ei = _oracle_check(st, oracle, rows, q, groups, 10, 1, n)
    assert len(ei) == 10 and sum(groups[i] == 0 for i in ei) == 1 and len(set(groups[ei].tolist())) == 10
    c, i, cnt = st.search_raw(q, 1024)
    post = cap_per_group(c[0][:cnt[0]], i[0][:cnt[0]], groups[i[0][:cnt[0]]], 10, 1)[1]
    assert len(post) < 10  # what capping after the ranking loses
    st.close()


@pytest.mark.parametrize("dim", [384, 100])
def test_ties_go_to_the_lower_id(VS, dim):
    n = 600
    rows = synth_rows(701 + dim, 0, n, dim)
    v = synth_rows(702 + dim, 0, 1, dim)[0]
    same = [10, 11, 12, 300, 301, 590]  # identical rows: inside one group (10, 11, 12) and across groups
    rows[same] = v
    groups = {r: 100 + r for r in range(n)}
    groups.update({10: 1, 11: 1, 12: 1, 300: 2, 301: 3, 590: 1})
    st = _store(VS, rows)
    st.set_groups(list(groups), list(groups.values()))
    truth = [_full_order(st, v)]
    assert truth[0][1][:6].tolist() == same
    qs = v[None, :]
    for k, m, want in [(2, 2, [10, 11]), (3, 2, [10, 11, 300]), (4, 2, [10, 11, 300, 301]), (2, 1, [10, 300]),
                       (1, 1, [10]), (3, 3, [10, 11, 12]), (5, 3, [10, 11, 12, 300, 301])]:
        _check(st, truth, _group_lookup(groups), qs, k, m)
        assert st.search_raw(qs, k, per_file=m)[1][0].tolist() == want
    for k, m in [(50, 1), (50, 2), (600, 2)]:
        _check(st, truth, _group_lookup(groups), qs, k, m)
    st.close()


def test_groups_follow_the_store_life_cycle(VS):
    n, dim, base = 900, 384, 1000
    rows = synth_rows(801, 0, n, dim)
    qs = synth_rows(802, 0, 2, dim)
    st = _store(VS, rows, id_base=base)
    groups = {base + r: r // 16 for r in range(n)}
    st.set_groups(list(groups), list(groups.values()))
    look = _group_lookup(groups)

    def check_all():
        truth = [_full_order(st, q) for q in qs]
        for k, m in [(10, 1), (40, 2), (200, 3)]:
            _check(st, truth, look, qs, k, m)
        return truth

    truth = check_all()
    # deleting a group's best row promotes its next one
    best = int(truth[0][1][0])
    mates = [int(i) for i in truth[0][1] if groups[int(i)] == groups[best]]
    assert st.search_raw(qs[0], 10, per_file=1)[1][0][0] == best
    assert st.delete_chunks([best]) == 1
    st.build_index()
    n_groups = len(set(groups.values()))
    c, i, cnt = st.search_raw(qs[0], 100, per_file=1)  # k above the number of groups: every group's best live row
    got = i[0][:cnt[0]].tolist()
    assert cnt[0] == n_groups and best not in got and mates[1] in got
    check_all()
    # a build that reclaims the deleted rows moves rows, not groups
    dead = [base + r for r in range(0, n, 5) if base + r != best]
    assert st.delete_chunks(dead) == len(dead)
    st.build_index()
    assert st.stored_rows() == len(st) == n - 1 - len(dead)
    check_all()
    # ids appended after set_groups are uncapped until they are assigned; an assignment needs no build
    new = st.insert_embeddings(np.stack([0.95 * qs[0] + 0.05 * rows[j] for j in range(6)])).tolist()
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    top6 = check_all()[0][1][:6].tolist()
    assert sorted(top6) == sorted(new)
    assert st.search_raw(qs[0], 10, per_file=1)[1][0][:6].tolist() == top6
    for i in new:
        groups[i] = 7000
    st.set_groups(new, [7000] * len(new))
    got = st.search_raw(qs[0], 10, per_file=1)[1][0].tolist()
    assert len(set(got) & set(new)) == 1
    check_all()
    # a deleted id is still an id; one never issued is not
    st.set_groups([best], [5])
    with pytest.raises(_lib.CsError, match="never issued"):
        st.set_groups([base - 1], [5])
    with pytest.raises(_lib.CsError, match="never issued"):
        st.set_groups([st.next_id()], [5])
    # clear drops the groups with the ids
    st.clear()
    assert st.groups_info()[0] == 0
    st.close()


def test_multi_level_capped_merge_over_1m_rows(VS, oracle):
    n, dim, seed, k, m = 1_000_000, 384, 0x6E0, 200, 8
    st = VS(None, dim)
    st.insert_synthetic(n, seed, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    groups = (np.arange(n) % 50).astype(np.uint32)
    st.set_groups(np.arange(n), groups)
    corpus = oracle.synth_rows(seed, 0, n, dim)
    qs = synth_rows(seed + 9, 0, 2, dim)
    cos, ids, cnt = st.search_raw(qs, k, per_file=m)
    for q in range(2):
        oc, oi = oracle.scan_topk(corpus, qs[q], 1024, mode="omp")
        ec, ei = cap_per_group(oc, oi, groups[oi], k, m)
        assert len(ei) >= k  # the oracle's 1,024 best hold the whole answer
        assert cnt[q] == k and ids[q].tolist() == ei
        assert np.abs(cos[q] - np.asarray(ec, np.float32)).max() < 1e-4
        # the answer lies inside the oracle's 1,024 best, which are the streaming search's 1,024 best: every cosine is
        # compared with that search's bits
        assert _same_bits_as_the_stream(st, qs[q], cos[q], ids[q]) == k
        one = st.search_raw(qs[q], k, per_file=m)  # one query per call: the deep / single-query launch, same three levels
        assert one[2][0] == k and one[1][0].tobytes() == ids[q].tobytes() and one[0][0].tobytes() == cos[q].tobytes()
    assert st.groups_info() == (n, 4 * n)
    st.close()


def test_concurrent_grouped_searches_and_errors(VS):
    n, dim, k = 60_000, 384, 25
    st = VS(None, dim)
    st.insert_synthetic(n, 0xC0C2, 0)
    q = synth_rows(0xC0C3, 0, 2, dim)
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.search_raw(q, k, per_file=1)
    st.build_index()
    with pytest.raises(_lib.CsError, match="Query embedding dimension mismatch: expected 384, got 100"):
        st.search_raw(np.zeros((1, 100), np.float32), 5, per_file=1)
    with pytest.raises(_lib.CsError, match="per_group must be at least 1"):
        st.search_raw(q, k, per_file=0)
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 1025"):
        st.search_raw(q, 1025, per_file=1)
    with pytest.raises(ValueError, match="exclusive"):
        st.search_raw(q, k, per_file=1, chunk_ids=[1])
    with pytest.raises(_lib.CsError, match="never issued"):
        st.set_groups([n], [1])
    st.set_groups(np.arange(n), np.arange(n) % 9)
    before = st.search_raw(q, k)
    caps = [1, 2, 3, 5]
    want = [st.search_raw(q, k, per_file=m) for m in caps]
    assert [int(w[2][0]) for w in want] == [9, 18, 25, 25]
    errors = []

    def work(t):
        try:
            for _ in range(6):
                r = st.search_raw(q, k, per_file=caps[t])
                if not all(x.tobytes() == y.tobytes() for x, y in zip(r, want[t])):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(len(caps))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    after = st.search_raw(q, k)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_files_are_groups_through_insert_reopen_and_clear(VS, tmp_path):
    """The path -> group layer of the Python store: chunks inserted with metadata are grouped by their file, a reopened
    store rebuilds the groups from its chunk sidecar, clear() starts the numbering again, and rows without metadata
    (insert_embeddings) are never capped."""
    dim, per = 384, 12
    files = ["vendor/gen.rs", "src/a.rs", "src/b.rs", "src/c.rs", "lib/d.rs"]
    q = synth_rows(901, 0, 1, dim)[0]
    noise = synth_rows(902, 0, per * len(files), dim)
    paths = [files[i % len(files)] for i in range(len(noise))]  # the files' chunks interleaved: groups are not id ranges
    rows = noise.copy()
    hog = [i for i, p in enumerate(paths) if p == files[0]]
    rows[hog] = 0.9 * q + 0.1 * noise[hog]  # one file of near-duplicates of the query
    by_id = dict(enumerate(paths))

    def check(st, id_paths, k=5):
        st.set_single_query_route(st.ROUTE_STREAM)
        assert st.groups_info()[0] == len(id_paths)
        full_c, full_i = _full_order(st, q)
        number = {}
        look = [number.setdefault(id_paths[int(i)], len(number)) if int(i) in id_paths else NO_GROUP for i in full_i]
        plain = st.search(q, k)
        assert {r.path for r in plain} == {files[0]}  # uncapped: the near-duplicates fill the list
        for m in (1, 2):
            want = cap_per_group(full_c, full_i, look, k * m, m)[1]
            got = st.search(q, k * m, per_file=m)
            assert [r.id for r in got] == want and [r.path for r in got] == [id_paths[i] for i in want]
            counts = {f: sum(r.path == f for r in got) for f in files}
            assert counts == {f: m for f in files}  # k * m hits over five files: m of each
            assert got[0].path == files[0]
        both = st.search_batch(np.stack([q, noise[3]]), k, per_file=1)
        assert [r.id for r in both[0]] == [r.id for r in st.search(q, k, per_file=1)]
        assert sorted(r.path for r in both[1]) == sorted(files) and both[1][0].path == files[3]

    db = tmp_path / "files.db"
    st = VS(db, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(len(paths)))
    st.build_index()
    check(st, by_id)
    st.close()

    st = VS(db, dim)  # reopened: the groups follow from the sidecar's paths
    check(st, by_id)
    # rows without metadata stay uncapped: six more near-duplicates all come back, beside one hit per file
    extra = st.insert_embeddings(np.stack([0.95 * q + 0.05 * noise[j] for j in range(6)])).tolist()
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.groups_info()[0] == len(paths)
    ids = st.search_raw(q, 11, per_file=1)[1][0].tolist()
    assert sorted(ids[:6]) == sorted(extra) and sorted(by_id[i] for i in ids[6:]) == sorted(files)
    assert len(st.search(q, 11, per_file=1)) == 5  # (results without metadata are skipped, as in every search)

    # clear() forgets the files' numbers with the ids; other paths, inserted in another order, are grouped afresh
    st.clear()
    assert st.groups_info()[0] == 0 and st._file_groups == {}
    order = np.random.default_rng(5).permutation(len(paths))
    again = [paths[i] for i in order]
    ids = st.insert_chunks_with_ids(_file_chunks(rows[order], again))
    st.build_index()
    check(st, dict(zip(ids, again)))
    st.close()

    sharded = VS(None, dim, devices=[0, 0])
    for call in (lambda: sharded.groups_info(), lambda: sharded.set_groups([0], [0])):
        with pytest.raises(_lib.CsError, match="sharded store has no grouped search"):
            call()
    sharded.close()


def test_cpp_wrapper_searches_per_file():
    """host/codesearch_gpu.hpp: VectorStore::set_groups and search_per_file (tests/cpp/grouped_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "grouped_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "grouped_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grouped host ok" in r.stdout
