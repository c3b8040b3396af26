"""Boosted search inside a scope (cs_index_search_boosted_scoped, codesearch_amd/csrc/scan_boosted.hip: the gathered
boosted scan): per query the exact best k rows of the scope by b = f32(score(cosine) * weight of the row's class), then id.

Ground truth comes only from code that exists without the feature: the full (cosine desc, id asc) order of the store — one
streaming search_raw(q, n) over at most 1,024 live rows, with its cosine bits — restricted to the scope's ids and passed
through search.boost_order.  Ids, the bytes of out_score and the bytes of out_cos must all match exactly."""
import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import boost_order
from codesearch_amd.synth import synth_rows
from codesearch_amd.vector_store import NO_CLASS

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF
f32 = np.float32
SHAPES = [(1, 1), (10, 1), (10, 3), (200, 9), (1000, 1), (10, 40)]  # (k, nq): test_gpu_boosted_search's


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _full_order(st, q):
    n = len(st)
    assert 0 < n <= 1024
    c, i, cnt = st.search_raw(q, n)
    assert cnt[0] == n
    return c[0].copy(), i[0].copy()


def _check(st, sc, inside, truth, classes, weights, qs, k):
    score, cos, ids, cnt = st.search_raw(qs, k, class_weights=weights, scope=sc)
    for q in range(qs.shape[0]):
        tc, ti = truth[q]
        keep = np.isin(ti, inside)
        tc, ti = tc[keep], ti[keep]
        es, ec, ei = boost_order(tc, ti, [classes.get(int(i), NO_CLASS) for i in ti], weights, k)
        n = len(ei)
        assert cnt[q] == n == min(k, len(ti)), (q, k, cnt[q], n)
        assert ids[q][:n].tolist() == ei.tolist(), (q, k)
        assert score[q][:n].tobytes() == es.tobytes(), (q, k)
        assert cos[q][:n].tobytes() == ec.tobytes(), (q, k)
        assert (ids[q][n:] == NO_ID).all() and (cos[q][n:] == 0).all() and (score[q][n:] == 0).all()


@pytest.mark.parametrize("dim", [384, 100])
def test_boosted_scoped_equals_boosted_scope_order(VS, dim):
    n, seed, base = 1000, 9600 + dim, 500
    rows = synth_rows(seed, 0, n, dim)
    qs = np.concatenate([synth_rows(seed + 1, 0, 38, dim), rows[[5, n - 3]]])
    st = VS(None, dim, id_base=base)
    st.insert_embeddings(rows)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    rng = np.random.default_rng(seed)
    all_ids = np.arange(base, base + n)
    sets = {
        "every id": all_ids,
        "a random 10 %": np.sort(rng.choice(all_ids, n // 10, replace=False)),
        "a contiguous block": all_ids[411:411 + 37],  # less than three deep tiles, an odd tail
        "one id": all_ids[[778]],
        "no id": all_ids[:0],
    }
    scopes = {name: st.scope(ids) for name, ids in sets.items()}
    classes = {int(i): int(i - base) % 18 for i in all_ids}
    st.set_classes(list(classes), list(classes.values()))
    tables = [np.where(np.arange(18) == 3, f32(1.15), f32(1.0)).astype(f32), rng.uniform(0.5, 1.5, 18).astype(f32),
              np.where(np.arange(18) == 5, f32(0.0), f32(1.0)).astype(f32), rng.uniform(0.5, 1.5, 7).astype(f32)]

    def check_all():
        truth = [_full_order(st, q) for q in qs]
        for name, sc in scopes.items():
            before = sc.route_info()
            for w in tables:
                for k, nq in SHAPES:
                    _check(st, sc, sets[name], truth, classes, w, qs[:nq], k)
            after = sc.route_info()
            if len(sets[name]):  # always the gathered route; an empty scope launches nothing
                assert after[0] == before[0] and after[1] == before[1] + len(tables) * len(SHAPES)

    check_all()
    # the scope holding every id answers as the unscoped call does
    a = st.search_raw(qs[:3], 25, class_weights=tables[1], scope=scopes["every id"])
    b = st.search_raw(qs[:3], 25, class_weights=tables[1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # the scopes outlive a build that reclaims deleted rows: their lists are remade, rows move, classes stay with the ids
    dead = all_ids[::3]
    assert st.delete_chunks(dead.tolist()) == len(dead)
    st.build_index()
    st.set_single_query_route(st.ROUTE_STREAM)
    assert st.stored_rows() == len(st) == n - len(dead)
    check_all()
    # the scope's own errors
    other = VS(None, dim)
    other.insert_embeddings(rows[:10])
    other.build_index()
    with pytest.raises(_lib.CsError, match="made for another store"):
        other.search_raw(qs[:1], 5, class_weights=tables[0], scope=scopes["one id"])
    other.close()
    lib = st._lib
    out = np.zeros((1, 5), np.uint32)
    rc = lib.cs_index_search_boosted_scoped(st.handle, None, qs.ctypes.data_as(_lib.f32p), 1, dim, 5, None, 0, None, None,
                                            out.ctypes.data_as(_lib.u32p), None)
    assert rc == _lib.CS_ERR_BAD_ARG and b"null scope" in lib.cs_last_error()
    for sc in scopes.values():
        sc.close()
    st.close()
