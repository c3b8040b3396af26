"""Boosted search (cs_index_search_boosted, codesearch_amd/csrc/scan_boosted.hip): the exact best k live rows by
b = f32(score(cosine) * weight of the row's class), then id — the exact form of the reference's kind and language boosts,
which re-weight only the hits it has already ranked (src/search/mod.rs:238-252, :789-806).

Ground truth comes only from code that exists without the feature: the full (cosine desc, id asc) order of a store of at
most 1,024 live rows — one streaming search_raw(q, n), with its cosine bits — passed through search.boost_order.  Ids, the
bytes of out_score and the bytes of out_cos must all match exactly."""
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import boost_order
from codesearch_amd.sharded import key_pack
from codesearch_amd.synth import synth_rows
from codesearch_amd.vector_store import CHUNK_KINDS, NO_CLASS, cos_to_score

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF
f32 = np.float32
SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1000, 1), (10, 40)]  # (k, nq)


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


def _class_lookup(classes: dict):
    return lambda ids: [classes.get(int(i), NO_CLASS) for i in ids]


def _check(st, truth, lookup, weights, qs, k, scope=None, inside=None):
    """st.search_raw(qs, k, class_weights=weights[, scope=]) against truth[q] = the full order of query q (restricted to the
    ids `inside` for a scope), boosted on the host."""
    score, cos, ids, cnt = st.search_raw(qs, k, class_weights=weights, scope=scope)
    for q in range(qs.shape[0]):
        tc, ti = truth[q]
        if inside is not None:
            keep = np.isin(ti, inside)
            tc, ti = tc[keep], ti[keep]
        es, ec, ei = boost_order(tc, ti, lookup(ti), weights, k)
        n = len(ei)
        assert cnt[q] == n, (q, k, cnt[q], n)
        assert ids[q][:n].tolist() == ei.tolist(), (q, k)
        assert score[q][:n].tobytes() == es.tobytes(), (q, k)
        assert cos[q][:n].tobytes() == ec.tobytes(), (q, k)
        assert (ids[q][n:] == NO_ID).all() and (cos[q][n:] == 0).all() and (score[q][n:] == 0).all()
    return score, cos, ids, cnt


def _kind_weights(kind, w):
    t = np.ones(len(CHUNK_KINDS), f32)
    t[kind] = w
    return t


@pytest.mark.parametrize("dim", [384, 768, 1024, 100])
def test_boosted_equals_boosted_full_order(VS, dim):
    n, seed = 1000, 9500 + dim
    rows = synth_rows(seed, 0, n, dim)
    qs = np.concatenate([synth_rows(seed + 1, 0, 38, dim), rows[[5, n - 3]]])
    st = _store(VS, rows)
    truth = [_full_order(st, q) for q in qs]
    assert st.classes_info() == (0, 0)
    rng = np.random.default_rng(seed)
    by_kind = {r: r % 18 for r in range(n)}
    classings = [
        ("none", {}, _kind_weights(3, 1.15)),
        ("kind at 1.15", by_kind, _kind_weights(3, 1.15)),
        ("63 classes, random weights", {r: r // 16 for r in range(n)}, rng.uniform(0.5, 1.5, 63).astype(f32)),
        ("one class weighs 0", by_kind, _kind_weights(5, 0.0)),
        ("a table shorter than the classes", by_kind, rng.uniform(0.5, 1.5, 7).astype(f32)),
    ]
    for name, classes, weights in classings:
        if classes:
            st.set_classes(list(classes), list(classes.values()))
            assert st.classes_info()[0] == n
        for k, nq in SHAPES:
            _check(st, truth, _class_lookup(classes), weights, qs[:nq], k)
        assert st.classes_info() == ((n, 2 * n) if classes else (0, 0))  # 2 B per id, from the first search on
    # no table at all: every row weighs 1 whatever its class
    _check(st, truth, _class_lookup(by_kind), np.zeros(0, f32), qs[:3], 10)
    st.close()


CLOSE = [0.99, 1.0, 1.01]  # within the spread of the best scores, so the answer mixes the classes


@pytest.mark.parametrize("n,k,values", [(20_000, 10, CLOSE), (20_000, 200, CLOSE), (120_000, 200, CLOSE),
                                        (120_000, 200, [0.25, 1.0, 1.5]), (600_000, 10, CLOSE), (600_000, 10, [0.0, 1.0, 4.0])])
def test_more_rows_than_one_streaming_search_returns(VS, n, k, values):
    """Three weight values over more rows than a search returns.  Truth for any store size: per weight value the scoped
    streaming top-k of the rows that carry it (exact bits), boosted on the host, merged by key_pack, the first k.
    From 100,000 rows on at k = 200, and from 500,000 at k = 10, the scan runs behind its prime pass."""
    dim = 384
    qs = synth_rows(9701, 0, 3, dim)
    st = VS(None, dim)
    st.insert_synthetic(n, 9700, 0)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    values = np.array(values, f32)
    cls = (np.arange(n) * 7 % 3).astype(np.uint16)
    st.set_classes(np.arange(n), cls)
    parts = []
    for c in range(3):
        sc = st.scope(np.flatnonzero(cls == c))
        sc.set_route("gather")
        pc, pi, pn = st.search_raw(qs, k, scope=sc)
        assert (pn == k).all()
        parts.append(((cos_to_score(pc) * values[c]).astype(f32), pc, pi))
        sc.close()
    score, cos, ids, cnt = st.search_raw(qs, k, class_weights=values)
    for q in range(len(qs)):
        b = np.concatenate([p[0][q] for p in parts])
        c = np.concatenate([p[1][q] for p in parts])
        i = np.concatenate([p[2][q] for p in parts])
        order = np.argsort(key_pack(b, i))[::-1][:k]
        assert cnt[q] == k and ids[q].tolist() == i[order].tolist()
        assert score[q].tobytes() == b[order].tobytes() and cos[q].tobytes() == c[order].tobytes()
        if values.tolist() == np.array(CLOSE, f32).tolist():
            assert len(set(cls[ids[q]].tolist())) > 1
    one = st.search_raw(qs[0], k, class_weights=values)  # one query per call: the deep / single-query launch
    assert all(x[0].tobytes() == y[0].tobytes() for x, y in zip(one, (score, cos, ids, cnt)))
    everything = st.scope(np.arange(n))  # the gathered form, behind its own prime pass from the same sizes on
    inside = st.search_raw(qs, k, class_weights=values, scope=everything)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(inside, (score, cos, ids, cnt)))
    everything.close()
    st.close()


def _chunks(rows, kind="Function"):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, kind, "src/a.rs"), rows[i]) for i in range(len(rows))]


def test_a_boosted_chunk_just_outside_the_list_rises_into_it(VS):
    """What the feature is for.  The chunk ranked k + 1 by cosine carries the boosted kind and its score * 1.15 beats the
    k-th score: the boosted search returns it; boosting the streaming top-k on the host, the reference's method, cannot."""
    n, dim, k = 500, 384, 10
    rows = synth_rows(9800, 0, n, dim)
    q = synth_rows(9801, 0, 1, dim)[0]
    st = VS(None, dim)
    ids = st.insert_chunks_with_ids(_chunks(rows))
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert ids == list(range(n)) and st.classes_info()[0] == n  # every chunk carries its kind
    tc, ti = _full_order(st, q)
    outsider = int(ti[k])
    struct = CHUNK_KINDS.index("Struct")
    assert cos_to_score(tc[k]) * f32(1.15) > cos_to_score(tc[k - 1])
    st.set_classes([outsider], [struct])  # (re-assigned: the chunk's metadata still says Function)
    classes = {i: CHUNK_KINDS.index("Function") for i in range(n)}
    classes[outsider] = struct
    w = _kind_weights(struct, f32(1.0) + f32(0.15))
    score, cos, got, cnt = _check(st, [(tc, ti)], _class_lookup(classes), w, q[None, :], k)
    assert outsider in got[0].tolist()
    sc, si, sn = st.search_raw(q, k)  # rank k, then boost
    post = boost_order(sc[0], si[0], _class_lookup(classes)(si[0]), w, k)[2]
    assert outsider not in post.tolist() and set(post.tolist()) == set(ti[:k].tolist())
    # the same through search(boost_kind=): score is b, distance the chunk's own
    res = st.search(q, k, boost_kind="Struct", boost=0.15)
    assert [r.id for r in res] == got[0].tolist()
    assert [f32(r.score) for r in res] == score[0].tolist()
    hit = [r for r in res if r.id == outsider][0]
    assert f32(hit.score) == f32(cos_to_score(tc[k]) * w[struct]) and f32(hit.distance) == f32((f32(1) - tc[k]) * f32(0.5))
    plain = st.search(q, k)
    assert [r.id for r in plain] == ti[:k].tolist()
    with pytest.raises(ValueError, match="CHUNK_KINDS"):
        st.search(q, k, boost_kind="Structure")
    with pytest.raises(ValueError, match="exclusive with per_file"):
        st.search(q, k, boost_kind="Struct", per_file=1)
    with pytest.raises(ValueError, match="exclusive with chunk_ids"):
        st.search_raw(q, k, class_weights=w, chunk_ids=[1, 2])
    st.close()


def test_unknown_kinds_carry_no_class(VS):
    dim = 384
    rows = synth_rows(9850, 0, 6, dim)
    st = VS(None, dim)
    st.insert_chunks_with_ids(_chunks(rows[:4], "Enum") + _chunks(rows[4:], "Gadget"))
    assert st.classes_info()[0] == 4
    st.close()


def test_classes_follow_the_store_life_cycle(VS):
    n, dim, base = 900, 384, 1000
    rows = synth_rows(9900, 0, n, dim)
    qs = synth_rows(9901, 0, 2, dim)
    st = _store(VS, rows, id_base=base)  # id_base != 0
    classes = {base + r: r % 18 for r in range(n)}
    st.set_classes(list(classes), list(classes.values()))
    weights = np.random.default_rng(3).uniform(0.5, 1.5, 18).astype(f32)
    look = _class_lookup(classes)

    def check_all():
        truth = [_full_order(st, q) for q in qs]
        out = [_check(st, truth, look, weights, qs, k) for k in (10, 40, 200)]
        _check(st, truth, look, weights, qs, len(st))  # every live row: each winner's row is found again
        return truth, out

    check_all()
    # a third of the rows deleted and reclaimed: row != id - id_base from here on (the bisection of the cosine pass)
    dead = [base + r for r in range(0, n, 3)]
    assert st.delete_chunks(dead) == len(dead)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.stored_rows() == len(st) == n - len(dead)
    assert st.classes_info()[0] == n  # builds and the reclaim leave the table alone
    check_all()
    # rows appended after set_classes weigh 1; an assignment needs no build and changes the next answer
    new = st.insert_embeddings(np.stack([0.95 * qs[0] + 0.05 * rows[j] for j in range(6)])).tolist()
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    truth, before = check_all()
    top = before[0][2][0][:6].tolist()
    assert sorted(top) == sorted(new)
    assert before[0][0][0][:6].tobytes() == cos_to_score(before[0][1][0][:6]).tobytes()  # b = s: weight 1
    heavy = int(np.argmax(weights))
    for i in new[:3]:
        classes[i] = heavy
    st.set_classes(new[:3], [heavy] * 3)
    _, after = check_all()
    assert after[0][2][0][:3].tolist() == sorted(new[:3], key=lambda i: top.index(i))
    assert not np.array_equal(after[0][0][0][:6], before[0][0][0][:6])
    # a deleted id is still an id; one never issued is not, and then nothing of the call is assigned
    st.set_classes([dead[0]], [5])
    have = st.classes_info()[0]
    for bad in (base - 1, st.next_id()):
        with pytest.raises(_lib.CsError, match="never issued"):
            st.set_classes([base + 1, bad], [NO_CLASS, 5])
        assert st.classes_info()[0] == have
    check_all()
    st.set_classes([base + 1], [NO_CLASS])  # un-assigns
    assert st.classes_info()[0] == have - 1
    # clear drops the table with the ids
    st.clear()
    assert st.classes_info() == (0, 0)
    st.close()


def test_arguments(VS):
    n, dim, k = 300, 384, 5
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(9950, 0, n, dim))
    q = synth_rows(9951, 0, 2, dim)
    ones = np.ones(4, f32)
    with pytest.raises(_lib.CsError, match="Index not built"):
        st.search_raw(q, k, class_weights=ones)
    st.build_index()
    with pytest.raises(_lib.CsError, match="Query embedding dimension mismatch: expected 384, got 100"):
        st.search_raw(np.zeros((1, 100), f32), k, class_weights=ones)
    with pytest.raises(_lib.CsError, match="k must be in 1..1024, got 1025"):
        st.search_raw(q, 1025, class_weights=ones)
    for bad in (np.nan, -0.5, np.inf, -np.inf, 65537.0):
        w = ones.copy()
        w[2] = bad
        with pytest.raises(_lib.CsError, match=r"weights\[2\]"):
            st.search_raw(q, k, class_weights=w)
    st.search_raw(q, k, class_weights=np.array([0.0, 65536.0], f32))  # the ends of the range are weights
    st.search_raw(q, k, class_weights=np.ones(4096, f32))
    with pytest.raises(_lib.CsError, match="n_classes must be at most 4096, got 4097"):
        st.search_raw(q, k, class_weights=np.ones(4097, f32))
    with pytest.raises(_lib.CsError, match="never issued"):
        st.set_classes([0, n], [1, 1])
    assert st.classes_info() == (0, 0)
    # each output is optional, but one must be given
    lib, h = st._lib, st.handle
    qp = q.ctypes.data_as(_lib.f32p)
    want = st.search_raw(q, k, class_weights=ones)
    ids = np.zeros((2, k), np.uint32)
    _lib.check(lib.cs_index_search_boosted(h, qp, 2, dim, k, None, 0, None, None, ids.ctypes.data_as(_lib.u32p), None))
    assert ids.tobytes() == want[2].tobytes()
    cos = np.zeros((2, k), f32)
    _lib.check(lib.cs_index_search_boosted(h, qp, 2, dim, k, None, 7, None, cos.ctypes.data_as(_lib.f32p), None, None))
    assert cos.tobytes() == want[1].tobytes()
    assert lib.cs_index_search_boosted(h, qp, 2, dim, k, None, 0, None, None, None, None) == _lib.CS_ERR_BAD_ARG
    # an empty store gives empty lists
    st.clear()
    st.build_index()
    score, cos, ids, cnt = st.search_raw(q, k, class_weights=ones)
    assert (cnt == 0).all() and (ids == NO_ID).all() and (cos == 0).all() and (score == 0).all()
    st.close()
    sharded = VS(None, dim, devices=[0, 0])
    for call in (lambda: sharded.classes_info(), lambda: sharded.set_classes([0], [0]),
                 lambda: sharded.search_raw(q, k, class_weights=ones)):
        with pytest.raises(_lib.CsError, match="sharded store has no boosted search"):
            call()
    sharded.close()


def test_two_threads_with_their_own_tables(VS):
    n, dim, k = 1000, 384, 25
    rows = synth_rows(9960, 0, n, dim)
    qs = synth_rows(9961, 0, 2, dim)
    st = _store(VS, rows)
    classes = {r: r % 18 for r in range(n)}
    st.set_classes(list(classes), list(classes.values()))
    truth = [_full_order(st, q) for q in qs]
    tables = [_kind_weights(3, 1.5), _kind_weights(11, 0.25)]
    want = [_check(st, truth, _class_lookup(classes), w, qs, k) for w in tables]
    assert want[0][2].tobytes() != want[1][2].tobytes()
    errors = []

    def work(t):
        try:
            for _ in range(20):
                r = st.search_raw(qs, k, class_weights=tables[t])
                if not all(x.tobytes() == y.tobytes() for x, y in zip(r, want[t])):
                    errors.append(t)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    st.close()
