"""Scoped similar-pairs search (cs_index_similar_pairs_scoped, codesearch_amd/csrc/scan_pairs_scoped.hip): every pair of
chunks above a cosine bound inside one scope or between two, exact — the scopes' rows packed into f16 buffers of the call's
own, joined on the f16 MFMA, the survivors re-scored in f32 by the unscoped call's refine.

Ground truth comes only from code that exists without the feature.  The primary truth is the unscoped call,
similar_pairs_raw(bound, max_pairs=65536), neither refused nor cut, reduced on the host by search.pairs_between.  Where the
unscoped call must be refused, the truth is similar_raw(sources in A, 1024, scope=B, exclude="self" | "file", min_cos=bound)
on the gathered route, no list reaching 1,024, merged on the host by search.pairs_above.  Ids, order, total and cosine bytes
must match exactly, and every returned pair has a < b.

Planted data as in test_gpu_similar_pairs.py (restated here): the background is synth_rows (no background pair at 1,000 x
384 exceeds 0.22); a pair at a target cosine c is rows[b] = |rows[b]| (c u + sqrt(1 - c^2) w) in float64; the deltas +-2e-4
and +-5e-4 around 0.9 lie inside the f16 filter's margin, so only the refine separates them."""
import ctypes
import re
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, pairs_above, pairs_between
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
BOUND = np.float32(0.9)
ROOM = 65536


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


def _plant(rows, a, b, c):
    u = rows[a].astype(np.float64)
    u /= np.linalg.norm(u)
    x = rows[b].astype(np.float64)
    w = x - (x @ u) * u
    w /= np.linalg.norm(w)
    rows[b] = (np.linalg.norm(x) * (c * u + np.sqrt(1.0 - c * c) * w)).astype(np.float32)


HUB, SPOKES = 600, [601, 602, 603, 604, 605, 640, 641, 642, 643, 644, 645]
TWINS = [990, 991, 992]  # identical rows, ungrouped
SPOTS = [(10, 20), (127, 128), (0, 999), (900, 950)]
DELTAS = [2e-4, -2e-4, 5e-4, -5e-4]
PLANTED = sorted({HUB, *SPOKES, *TWINS, *[r for p in SPOTS for r in p]})


def _planted(dim, rot=0, n=1000, extra=()):
    """-> (rows, near): `near` = the four pairs around the bound as (a, b, delta); rot moves the deltas over the spots;
    extra: further (a, b, cosine) to plant."""
    rows = synth_rows(7100 + dim, 0, n, dim).copy()
    near = []
    for s, (a, b) in enumerate(SPOTS):
        d = DELTAS[(s + rot) % 4]
        _plant(rows, a, b, float(BOUND) + d)
        near.append((a, b, d))
    for b in SPOKES:
        _plant(rows, HUB, b, 0.97)  # mutual cosines ~ 0.94: 66 pairs among the twelve rows
    rows[TWINS[1]] = rows[TWINS[0]]
    rows[TWINS[2]] = rows[TWINS[0]]
    for a, b, c in extra:
        _plant(rows, a, b, c)
    return rows, near


def _files_of_8(n, ungrouped, base=0):
    return {base + r: r // 8 for r in range(n - ungrouped)}


def _lookup(groups):
    return lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]


def _same(x, y):
    """Two answers (cos, a, b, total): the same bytes."""
    return x[3] == y[3] and all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[:3], y[:3]))


def _pairs(r):
    return list(zip(r[1].tolist(), r[2].tolist()))


def _full(st, bound, other):
    """The primary truth's source: the unscoped answer, neither refused nor cut."""
    full = st.similar_pairs_raw(bound, other_files=other, max_pairs=ROOM)
    assert full[3] <= ROOM and len(full[0]) == full[3]
    return full


def _check(st, sa, sb, ids_a, ids_b, bound, other, max_pairs=ROOM, full=None):
    """The scoped call (sb None: inside sa) against the unscoped answer reduced by pairs_between, bit for bit."""
    full = _full(st, bound, other) if full is None else full
    want = pairs_between(full[0], full[1], full[2], ids_a, ids_a if ids_b is None else ids_b)
    got = st.similar_pairs_raw(bound, other_files=other, max_pairs=max_pairs, scope=sa, other=sb)
    assert got[3] == want[3], (got[3], want[3])
    m = min(want[3], max_pairs)
    assert len(got[0]) == len(got[1]) == len(got[2]) == m
    assert got[1].tolist() == want[1][:m].tolist() and got[2].tolist() == want[2][:m].tolist()
    assert got[0].tobytes() == want[0][:m].tobytes()
    assert (got[1] < got[2]).all()
    info = st.similar_pairs_info()
    assert info["candidates"] >= got[3]
    return got


@pytest.mark.parametrize("dim,rot", [(384, 0), (768, 1), (1024, 2)])
def test_every_id_twice_is_the_unscoped_call(VS, dim, rot):
    n = 1000
    rows, near = _planted(dim, rot)
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    every = st.scope(range(n))
    twin = st.scope(range(n))
    for other, total in ((False, 71), (True, 71 - 30)):
        full = _full(st, BOUND, other)
        assert full[3] == total
        for sb in (None, every, twin):  # the triangle; the same handle named twice; the rectangle of two equal lists
            got = st.similar_pairs_raw(BOUND, other_files=other, scope=every, other=sb)
            assert _same(got, full), (other, sb)
        info = st.similar_pairs_info()
        assert info["bands"] == 1 and info["rows_a"] == info["rows_b"] == n and info["tile_pairs"] == 64
    got = st.similar_pairs_raw(BOUND, scope=every)
    assert st.similar_pairs_info()["tile_pairs"] == 36  # one handle: the triangle of 8 packed tiles
    have = set(_pairs(got))
    for pa, pb, d in near:  # the refine, not the filter, decided these
        assert ((pa, pb) in have) == (d > 0)
    assert every.route_info()[:3] == (0, 0, 0)  # not a search: the scopes' counters do not move
    low = np.float32(0.15)  # more of the background comes in, still exact
    assert _same(st.similar_pairs_raw(low, scope=every), _full(st, low, False))
    assert _same(st.similar_pairs_raw(low, other_files=True, scope=every, other=twin), _full(st, low, True))
    st.close()


@pytest.mark.parametrize("dim,rot", [(384, 0), (768, 1), (1024, 2)])
def test_packed_positions_differ_from_stored_rows(VS, dim, rot):
    """A scope of every third id plus the planted rows: packed row i is not stored row i.  A pair just above the bound is
    planted on the ids that land at packed positions 127 and 128 — the edge between the scope's first two packed tiles,
    which is no tile edge of the store — and one just under it on 126 and 129."""
    n = 1000
    ids = sorted(set(range(0, n, 3)) | set(PLANTED))
    e126, e127, e128, e129 = ids[126:130]
    assert not {e126, e127, e128, e129} & set(PLANTED) and e127 // 128 == e128 // 128
    rows, near = _planted(dim, rot, extra=[(e127, e128, float(BOUND) + 2e-4), (e126, e129, float(BOUND) - 2e-4)])
    assert ids.index(e127) == 127 and ids.index(e128) == 128  # asserted from the id list itself
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    third, every = st.scope(ids), st.scope(range(n))
    for other in (False, True):
        full = _full(st, BOUND, other)
        got = _check(st, third, None, ids, None, BOUND, other, full=full)
        reported = not other or groups[e127] != groups[e128]  # (files of 8 ids: the two may share one)
        assert ((e127, e128) in set(_pairs(got))) == reported and (e126, e129) not in set(_pairs(got))
        # against everything: the pairs with at least one end in the scope, the scope on the A side (it is the smaller)
        wide = _check(st, third, every, ids, range(n), BOUND, other, full=full)
        assert set(_pairs(got)) <= set(_pairs(wide)) and ((e127, e128) in set(_pairs(wide))) == reported
    assert st.similar_pairs_info()["rows_a"] == len(ids) and st.similar_pairs_info()["rows_b"] == n
    assert _pairs(_check(st, third, None, ids, None, BOUND, False))[:3] == [(990, 991), (990, 992), (991, 992)]
    _check(st, third, None, ids, None, np.float32(0.15), False)
    st.close()


@pytest.fixture(scope="module", params=[384, 768, 1024])
def small(VS, request):
    """300 background rows at each of the filter's dims: the unscoped full join is 44,850 pairs, inside the room of one
    call."""
    n = 300
    st = _store(VS, synth_rows(7200 + n + request.param, 0, n, request.param))
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    full = {other: _full(st, NEG_INF, other) for other in (False, True)}
    assert full[False][3] == n * (n - 1) // 2
    yield st, full
    st.close()


@pytest.mark.parametrize("m", [1, 2, 128, 129, 300])
def test_full_joins_inside_a_scope_without_a_bound(small, m):
    st, full = small
    ids = sorted(np.random.default_rng(m).choice(300, m, replace=False).tolist())
    with st.scope(ids) as sc:
        for bound in (NEG_INF, None):
            got = _check(st, sc, None, ids, None, bound, False, full=full[False])
            assert got[3] == m * (m - 1) // 2 == len(got[0])
        assert (np.diff(got[0]) <= 0).all()
        _check(st, sc, None, ids, None, NEG_INF, True, full=full[True])
        if m == 1:
            assert st.similar_pairs_info()["bands"] == 0  # one row holds no pair: nothing was launched


@pytest.mark.parametrize("inside", [True, False])
def test_129_by_1_and_1_by_129(small, inside):
    st, full = small
    ids = sorted(np.random.default_rng(9).choice(300, 129, replace=False).tolist())
    lone = [ids[70]] if inside else [next(i for i in range(300) if i not in set(ids))]
    with st.scope(ids) as wide, st.scope(lone) as one, st.scope(lone) as one_again:
        x = _check(st, wide, one, ids, lone, NEG_INF, False, full=full[False])
        y = _check(st, one, wide, lone, ids, NEG_INF, False, full=full[False])
        assert _same(x, y) and x[3] == (128 if inside else 129)
        assert lone[0] in set(x[1].tolist()) | set(x[2].tolist())
        info = st.similar_pairs_info()
        assert (info["rows_a"], info["rows_b"], info["tile_pairs"], info["bands"]) == (1, 129, 2, 1)
        # two handles that hold the same single row: no pair, and no launch
        assert st.similar_pairs_raw(NEG_INF, scope=one, other=one_again)[3] == 0
        assert st.similar_pairs_info()["bands"] == 0


@pytest.mark.parametrize("dim", [384, 768, 1024])
def test_two_scopes(VS, dim):
    n = 1000
    rows, near = _planted(dim)  # (10, 20) +2e-4, (127, 128) -2e-4, (0, 999) +5e-4, (900, 950) -5e-4
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    full = {other: _full(st, BOUND, other) for other in (False, True)}
    clique = {(a, b) for a in [HUB] + SPOKES for b in [HUB] + SPOKES if a < b}
    # disjoint: a planted pair across, (10, 20) inside A, the clique and the identical rows inside B — only the first is reported
    A, B = list(range(0, 500)), list(range(500, n))
    sa, sb = st.scope(A), st.scope(B)
    got = _check(st, sa, sb, A, B, BOUND, False, full=full[False])
    assert _pairs(got) == [(0, 999)] and got[3] == 1
    assert _same(got, _check(st, sb, sa, B, A, BOUND, False, full=full[False]))  # swapped: identical bytes
    _check(st, sa, sb, A, B, BOUND, True, full=full[True])
    # overlapping: the clique and the identical rows inside the intersection, (0, 999) from A \ B to B \ A, (10, 20) in A \ B
    A2, B2 = sorted(set(range(0, 650)) | set(TWINS)), list(range(600, n))
    assert set([HUB] + SPOKES + TWINS) <= set(A2) & set(B2) and 0 not in B2 and 999 not in A2 and 20 not in B2
    sa2, sb2 = st.scope(A2), st.scope(B2)
    got = _check(st, sa2, sb2, A2, B2, BOUND, False, full=full[False])
    have = _pairs(got)
    assert have[:3] == [(990, 991), (990, 992), (991, 992)] and got[0][0].tobytes() == got[0][1].tobytes() == got[0][2].tobytes()
    assert got[3] == 66 + 3 + 1 == len(set(have)) and clique <= set(have)  # every pair of the intersection once
    assert (0, 999) in have and (10, 20) not in have
    assert _same(got, _check(st, sb2, sa2, B2, A2, BOUND, False, full=full[False]))
    other = _check(st, sa2, sb2, A2, B2, BOUND, True, full=full[True])
    assert other[3] == 66 - 30 + 3 + 1
    # B inside A: every pair with an end in B, those inside B once
    B3 = list(range(600, 650))
    every, sb3 = st.scope(range(n)), st.scope(B3)
    got = _check(st, every, sb3, range(n), B3, BOUND, False, full=full[False])
    assert set(_pairs(got)) == clique
    assert _same(got, _check(st, sb3, every, B3, range(n), BOUND, False, full=full[False]))
    # two handles with equal ids: the bytes of one handle passed twice
    sa2_again = st.scope(A2)
    inside = _check(st, sa2, None, A2, None, BOUND, False, full=full[False])
    assert _same(inside, st.similar_pairs_raw(BOUND, scope=sa2, other=sa2_again))
    assert _same(inside, st.similar_pairs_raw(BOUND, scope=sa2_again, other=sa2))
    assert (10, 20) in _pairs(inside) and (0, 999) not in _pairs(inside)
    # a lower bound lets the background in on every form
    low = _full(st, np.float32(0.15), False)
    _check(st, sa2, sb2, A2, B2, np.float32(0.15), False, full=low)
    _check(st, sa, sb, A, B, np.float32(0.15), False, full=low)
    st.close()


def _gathered_truth(st, ids_a, scope_b, look, bound, other, max_pairs):
    """The second truth, for one scope joined with itself: per source of the scope, the similar-chunk search through the
    scope (always the gathered scan), merged by pairs_above (which takes each pair from its lower id)."""
    ids_a = [int(i) for i in ids_a]
    cos, hit, cnt = st.similar_raw(ids_a, 1024, exclude="file" if other else "self", min_cos=bound, scope=scope_b)
    assert (cnt < 1024).all()  # no list reached 1,024
    orders = {a: (cos[q][:cnt[q]].copy(), hit[q][:cnt[q]].copy()) for q, a in enumerate(ids_a)}
    return pairs_above(orders, look, "other_group" if other else "all", bound, max_pairs)


def test_a_scope_lifts_the_refusal_a_file_of_near_duplicates_causes(VS):
    """600 of 1,000 rows are near-duplicates of one row, all in one file (the hog of test_gpu_similar_pairs.py), plus two
    planted pairs among the 400 other rows.  The unscoped ALL call at max_pairs = 2,000 is refused; the scoped one over
    the 400 others is not, and a scope that contains the hog is refused with the same text."""
    n, dim = 1000, 384
    rows = synth_rows(7401, 0, n, dim).copy()
    hog = np.arange(200, 800)
    rows[hog[1:]] = 0.95 * rows[200] + 0.05 * rows[hog[1:]]
    rows[900] = 0.95 * rows[200] + 0.05 * rows[900]
    _plant(rows, 50, 60, 0.95)
    _plant(rows, 100, 850, 0.92)
    groups = {r: 1000 + r // 8 for r in range(n)}
    groups.update({int(r): 7 for r in hog})
    st = _store(VS, rows)
    st.set_groups(list(groups), list(groups.values()))
    with pytest.raises(_lib.CsError, match="candidate pairs") as e:
        st.similar_pairs_raw(BOUND, other_files=False, max_pairs=2000)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    refusal = str(e.value)
    others = [r for r in range(n) if r < 200 or r >= 800]
    assert len(others) == 400
    sc = st.scope(others)
    for other in (False, True):
        want = _gathered_truth(st, others, sc, _lookup(groups), BOUND, other, 2000)
        got = st.similar_pairs_raw(BOUND, other_files=other, max_pairs=2000, scope=sc)
        assert got[3] == want[3] == 2 and got[1].tolist() == want[1] and got[2].tolist() == want[2]
        assert got[0].tobytes() == np.asarray(want[0], np.float32).tobytes() and (got[1] < got[2]).all()
        assert _pairs(got) == [(50, 60), (100, 850)]
    # against a third of the hog: still inside the room (the 200 hog rows pair with row 900 only)
    part = others + list(range(200, 400))
    sp = st.scope(list(range(200, 400)))
    got = st.similar_pairs_raw(BOUND, max_pairs=2000, scope=sc, other=sp)
    assert got[3] == 200 and (got[2] == 900).all() and sorted(got[1].tolist()) == list(range(200, 400)) and len(part) == 600
    # a scope that contains the hog is refused like the unscoped call
    every = st.scope(range(n))
    mask = lambda t: re.sub(r"\d+ candidate pairs", "N candidate pairs", t)
    for kw in (dict(scope=every), dict(scope=every, other=st.scope(range(n))), dict(scope=st.scope(hog.tolist()))):
        with pytest.raises(_lib.CsError, match="candidate pairs") as e:
            st.similar_pairs_raw(BOUND, other_files=False, max_pairs=2000, **kw)
        assert e.value.code == _lib.CS_ERR_UNSUPPORTED and mask(str(e.value)) == mask(refusal)
    assert "8096" in refusal and "raise min_cos, exclude groups" in refusal and "raise max_pairs" in refusal
    # ... and the handle lives on
    assert st.similar_pairs_raw(BOUND, max_pairs=2000, scope=sc)[3] == 2
    st.close()


def test_id_base_deleted_rows_and_the_refresh(VS, monkeypatch):
    """id_base = 1,000; the scopes are made before 30 % of the rows are deleted; both states a built index can be in
    (tombstones kept: CS_INDEX_COMPACT_DEAD_PCT=0; reclaimed: the rows move, the ids stay).  The call refreshes the lists."""
    n, base = 1000, 1000
    rows, near = _planted(384)
    groups = _files_of_8(n, 40, base)
    kept = [(a, b) for a, b, d in near if d > 0]
    victim = base + kept[0][1]
    rng = np.random.default_rng(5)
    protect = {base + r for r in PLANTED}
    pool = [base + r for r in range(n) if base + r not in protect]
    gone = sorted(set(rng.choice(pool, (3 * n) // 10 - 1, replace=False).tolist()) | {victim})
    assert len(gone) == (3 * n) // 10
    all_ids = [base + r for r in range(n)]
    third = sorted({base + r for r in range(0, n, 3)} | protect)
    upper = [base + r for r in range(500, n)]
    answers = []
    for reclaim in (False, True):
        if not reclaim:
            monkeypatch.setenv("CS_INDEX_COMPACT_DEAD_PCT", "0")
        else:
            monkeypatch.delenv("CS_INDEX_COMPACT_DEAD_PCT")
        st = _store(VS, rows, id_base=base)
        st.set_groups(list(groups), list(groups.values()))
        every, s3, sup = st.scope(all_ids), st.scope(third), st.scope(upper)
        doomed = st.scope(gone[:20] + [base + n + 5, base + n + 9])  # ids about to be deleted, and two never issued
        full = _full(st, BOUND, False)
        got = _check(st, every, None, all_ids, None, BOUND, False, full=full)
        assert got[3] == 71 and (base + kept[0][0], victim) in set(_pairs(got)) and got[1].min() >= base
        _check(st, s3, sup, third, upper, BOUND, False, full=full)
        assert st.similar_pairs_raw(NEG_INF, scope=doomed)[3] == 190  # 20 live rows; the never-issued ids hold none
        made = [s.info()[2] for s in (every, s3, sup, doomed)]
        assert made == [1, 1, 1, 1]
        assert st.delete_chunks(gone) == len(gone)
        with pytest.raises(_lib.CsError, match="Index not built"):
            st.similar_pairs_raw(BOUND, scope=every)
        st.build_index()
        st.set_single_query_route(st.ROUTE_STREAM)
        assert st.stored_rows() == (n - len(gone) if reclaim else n) and len(st) == n - len(gone)
        assert [s.info()[2] for s in (every, s3, sup, doomed)] == made  # nothing refreshed yet
        full = _full(st, BOUND, False)
        got = _check(st, every, None, all_ids, None, BOUND, False, full=full)
        assert every.info() == (n, n - len(gone), 2)  # the call remade the list
        assert got[3] == 70 and victim not in set(got[1].tolist()) | set(got[2].tolist())
        assert _same(got, full)
        between = _check(st, s3, sup, third, upper, BOUND, False, full=full)
        assert s3.info()[2] == 2 and sup.info()[2] == 2
        inside = _check(st, s3, None, third, None, BOUND, True, full=_full(st, BOUND, True))
        low = _check(st, s3, every, third, all_ids, np.float32(0.15), False)
        # only deleted and never-issued ids: total 0, no launch — and the list was still refreshed
        assert st.similar_pairs_raw(NEG_INF, scope=doomed)[3] == 0 and st.similar_pairs_info()["bands"] == 0
        assert st.similar_pairs_raw(NEG_INF, scope=doomed, other=every)[3] == 0 and st.similar_pairs_info()["bands"] == 0
        assert st.similar_pairs_raw(NEG_INF, scope=every, other=doomed)[3] == 0 and st.similar_pairs_info()["bands"] == 0
        assert doomed.info() == (22, 0, 2)
        answers.append([x.tobytes() for r in (got, between, inside, low) for x in r[:3]])
        st.close()
    assert answers[0] == answers[1]  # tombstoned or reclaimed: the same pairs, the same bits


def test_repeat_and_no_trace_where_the_int8_copy_serves(VS):
    """5,000 rows: the int8 copy serves the index, which holds no f16 copy — the call packs its own buffers and leaves the
    index as it was: the same filter state and copies, the same bits from a search on the default route."""
    n, dim = 5000, 384
    rows = synth_rows(7501, 0, n, dim).copy()
    spots = [(5, 4999), (127, 128), (3000, 3001), (4990, 4995), (2047, 2048)]
    for i, (a, b) in enumerate(spots):
        _plant(rows, a, b, 0.9 + [2e-4, -2e-4, 5e-4, -5e-4, 0.05][i])
    st = VS(None, dim)
    st.insert_embeddings(rows)
    st.build_index()
    groups = _files_of_8(n, 40)
    st.set_groups(list(groups), list(groups.values()))
    assert st.filter_state()[0] == 2 and st.filter_copies()[:2] == (True, False)
    odd = sorted(set(range(1, n, 2)) | {r for p in spots for r in p})
    tail = list(range(2000, n))
    s_odd, s_tail = st.scope(odd), st.scope(tail)
    qs = synth_rows(7502, 0, 6, dim)
    state, copies, before = st.filter_state(), st.filter_copies(), st.search_raw(qs, 10)
    first = st.similar_pairs_raw(BOUND, scope=s_odd)
    assert first[3] == 3 and _pairs(first) == [(2047, 2048), (3000, 3001), (5, 4999)]
    cross = st.similar_pairs_raw(BOUND, scope=s_odd, other=s_tail)
    assert _pairs(cross) == [(2047, 2048), (3000, 3001), (5, 4999)]
    for _ in range(2):  # the same calls three times: identical bytes
        assert _same(first, st.similar_pairs_raw(BOUND, scope=s_odd))
        assert _same(cross, st.similar_pairs_raw(BOUND, scope=s_odd, other=s_tail))
    assert st.filter_state() == state and st.filter_copies() == copies
    after = st.search_raw(qs, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    for other in (False, True):
        full = _full(st, BOUND, other)
        _check(st, s_odd, None, odd, None, BOUND, other, full=full)
        _check(st, s_odd, s_tail, odd, tail, BOUND, other, full=full)
        _check(st, s_tail, None, tail, None, BOUND, other, full=full)
    assert st.filter_state() == state and st.filter_copies() == copies
    st.close()


def test_the_bound_is_strict_and_truncation_keeps_the_total(VS):
    rows, near = _planted(384)
    st = _store(VS, rows)
    ids = sorted(set(range(0, 1000, 3)) | set(PLANTED))
    sc, every = st.scope(ids), st.scope(range(1000))
    full = _full(st, BOUND, False)
    whole = _check(st, sc, None, ids, None, BOUND, False, full=full)
    assert whole[3] == 71
    for room in (1, 10):
        cut = _check(st, sc, None, ids, None, BOUND, False, max_pairs=room, full=full)
        assert cut[3] == 71 and len(cut[1]) == room and cut[0].tobytes() == whole[0][:room].tobytes()
        cut = _check(st, sc, every, ids, range(1000), BOUND, False, max_pairs=room, full=full)
        assert cut[3] == 71 and len(cut[1]) == room
    assert _pairs(st.similar_pairs_raw(BOUND, max_pairs=1, scope=sc)) == [(990, 991)]
    pa, pb = [(a, b) for a, b, d in near if d == 2e-4][0]
    cos, hit, cnt = st.similar_raw([pa], 1024, exclude="self", min_cos=0.5)
    exact = np.float32(cos[0][hit[0][:cnt[0]].tolist().index(pb)])  # the pair's f32 cosine, from the similar-chunk search
    assert abs(float(exact) - 0.9002) < 1e-6
    for sb, ids_b in ((None, None), (every, range(1000))):
        at = _check(st, sc, sb, ids, ids_b, exact, False)
        assert (pa, pb) not in set(_pairs(at)) and at[3] == 70
        below = _check(st, sc, sb, ids, ids_b, np.nextafter(exact, np.float32(-1)), False)
        assert (pa, pb) in set(_pairs(below)) and below[3] == 71
        assert below[0][_pairs(below).index((pa, pb))].tobytes() == exact.tobytes()
    assert st.similar_pairs_raw(2.0, scope=sc)[3] == 0  # above every cosine
    st.close()


def _raw(lib, h, sa, sb, min_cos, mode, max_pairs, a, b, cos, total):
    p = lambda x, t: x.ctypes.data_as(t) if x is not None else None
    return lib.cs_index_similar_pairs_scoped(h, sa, sb, min_cos, mode, max_pairs, p(a, _lib.u32p), p(b, _lib.u32p),
                                             p(cos, _lib.f32p), ctypes.byref(total) if total is not None else None)


class _Out:
    """Output buffers prefilled with a pattern: a failing call writes nothing."""

    def __init__(self, room):
        self.a = np.full(room, 0xA5A5A5A5, np.uint32)
        self.b = np.full(room, 0x5A5A5A5A, np.uint32)
        self.cos = np.full(room, 7.0, np.float32)
        self.total = ctypes.c_uint64(0x7777)

    def untouched(self):
        return ((self.a == 0xA5A5A5A5).all() and (self.b == 0x5A5A5A5A).all() and (self.cos == 7.0).all()
                and self.total.value == 0x7777)


def test_errors_and_their_order(VS, gpu_lib, monkeypatch):
    n, dim = 500, 384
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(7601, 0, n, dim))
    elsewhere = _store(VS, synth_rows(7605, 0, 64, dim))
    sc, foreign = st.scope(range(0, n, 2)), elsewhere.scope(range(64))
    o = _Out(8)
    nan = float("nan")
    H = lambda s: s.handle if s is not None else None

    def fails(code, text, sa, sb, *args, handle=True):
        before = [s.info()[2] for s in (sc, foreign)]
        assert _raw(gpu_lib, st.handle if handle else None, H(sa), H(sb), *args) == code
        assert text in _lib.last_error(), _lib.last_error()
        assert o.untouched()                                        # a failing call writes nothing
        assert [s.info()[2] for s in (sc, foreign)] == before       # and refreshes no list

    bad = _lib.CS_ERR_BAD_ARG
    # 1. the unscoped call's, in its order, each before everything behind it (null and foreign scopes included)
    fails(bad, "null index handle", None, None, nan, 9, 0, None, None, None, None, handle=False)
    fails(_lib.CS_ERR_NOT_BUILT, "Index not built. Call build_index() after inserting chunks.", None, None, nan, 9, 0, None,
          None, None, None)
    st.build_index()
    fails(bad, "null buffer", None, None, nan, 9, 0, None, o.b, o.cos, o.total)
    fails(bad, "null buffer", sc, sc, nan, 9, 0, o.a, None, o.cos, o.total)
    fails(bad, "null buffer", sc, foreign, nan, 9, 0, o.a, o.b, None, o.total)
    fails(bad, "null buffer", None, sc, nan, 9, 0, o.a, o.b, o.cos, None)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", None, None, nan, 2, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", sc, sc, nan, -1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "min_cos is NaN", None, foreign, nan, 1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "max_pairs must be in 1..4194304, got 0", None, None, 0.5, 1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "max_pairs must be in 1..4194304, got 4194305", foreign, None, 0.5, 0, _lib.CS_MAX_PAIRS + 1, o.a, o.b, o.cos,
          o.total)
    # 2. a null scope_a, then a null scope_b: the text says which.  NULL does not mean "the whole store"
    fails(bad, "null scope handle (scope_a)", None, None, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    fails(bad, "null scope handle (scope_a)", None, foreign, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    fails(bad, "null scope handle (scope_b)", sc, None, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    fails(bad, "null scope handle (scope_b)", foreign, None, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    # 3. a scope made for another store, on either side
    fails(bad, "the scope was made for another store", foreign, sc, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    fails(bad, "the scope was made for another store", sc, foreign, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    fails(bad, "the scope was made for another store", foreign, foreign, 0.5, 0, 8, o.a, o.b, o.cos, o.total)
    assert sc.info()[2] == 0  # the list is still to be made: no failing call made it
    assert _raw(gpu_lib, st.handle, sc.handle, sc.handle, 0.5, 1, 8, o.a, o.b, o.cos, o.total) == _lib.CS_OK
    assert o.total.value == 0 and sc.info()[2] == 1 and sc.route_info()[:3] == (0, 0, 0)
    # 4. a dim the f16 filter has no tiles for — behind max_pairs and behind the scopes
    odd = VS(None, 100)
    odd.insert_embeddings(synth_rows(7602, 0, 50, 100))
    odd.build_index()
    so = odd.scope(range(50))
    made = so.info()[2]  # (a scope made over a built index has its list already)
    o = _Out(8)
    call = lambda sa, sb, room: _raw(gpu_lib, odd.handle, H(sa), H(sb), 0.5, 0, room, o.a, o.b, o.cos, o.total)
    assert call(so, so, 0) == bad and "max_pairs must be" in _lib.last_error()
    assert call(so, None, 8) == bad and "null scope handle (scope_b)" in _lib.last_error()
    assert call(so, sc, 8) == bad and "the scope was made for another store" in _lib.last_error()
    assert call(so, so, 8) == _lib.CS_ERR_UNSUPPORTED
    assert "dim 384, 768 or 1024" in _lib.last_error() and "got 100" in _lib.last_error() and o.untouched()
    assert so.info()[2] == made
    odd.close()
    # 5. CS_INDEX_SPLIT=0 turned the filter copies off: refused like the unscoped call, before the list is made
    monkeypatch.setenv("CS_INDEX_SPLIT", "0")
    off = VS(None, dim)
    off.insert_embeddings(synth_rows(7603, 0, 50, dim))
    off.build_index()
    sf = off.scope(range(50))
    made = sf.info()[2]
    assert _raw(gpu_lib, off.handle, sf.handle, sf.handle, 0.5, 0, 8, o.a, o.b, o.cos, o.total) == _lib.CS_ERR_UNSUPPORTED
    assert "CS_INDEX_SPLIT=0" in _lib.last_error() and o.untouched() and sf.info()[2] == made
    with pytest.raises(_lib.CsError, match="CS_INDEX_SPLIT=0"):
        off.similar_pairs_raw(0.5)
    off.close()
    monkeypatch.delenv("CS_INDEX_SPLIT")
    # the Python layer
    with pytest.raises(ValueError, match="other= needs scope="):
        st.similar_pairs_raw(0.9, other=sc)
    with pytest.raises(_lib.CsError, match="the scope was made for another store"):
        st.similar_pairs_raw(0.9, scope=sc, other=foreign)
    done = st.scope([1, 2])
    done.close()
    with pytest.raises(_lib.CsError, match="scope is closed"):
        st.similar_pairs_raw(0.9, scope=done)
    st.close()
    elsewhere.close()


def test_a_sharded_store_and_its_scopes_are_refused(VS):
    dim = 384
    st = _store(VS, synth_rows(9933, 0, 64, dim))
    sharded = VS(None, dim, devices=[0, 0])
    sharded.insert_embeddings(synth_rows(9934, 0, 64, dim))
    sharded.build_index()
    over_shards = sharded.scope(np.arange(64))
    with pytest.raises(_lib.CsError, match="no similar-pairs search: no cs_shards_ form yet") as e:
        sharded.similar_pairs_raw(0.9, scope=over_shards)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    mine = st.scope(np.arange(64))
    for kw in (dict(scope=over_shards), dict(scope=mine, other=over_shards), dict(scope=over_shards, other=mine)):
        with pytest.raises(_lib.CsError, match="the scope was made for another store") as e:
            st.similar_pairs_raw(0.9, **kw)
        assert e.value.code == _lib.CS_ERR_BAD_ARG
    sharded.close()
    st.close()


@pytest.mark.parametrize("n", [1000, 5000])  # whichever copy serves the index, the call packs buffers of its own
def test_no_room_for_the_packed_buffers(lab_lib, VS, monkeypatch, n):
    monkeypatch.setenv("CS_FAULT_F16_ALLOC", "1")
    st = VS(None, 384)
    st.insert_embeddings(synth_rows(7604, 0, n, 384))
    st.build_index()
    sc, half = st.scope(range(n)), st.scope(range(0, n, 2))
    for kw in (dict(scope=sc), dict(scope=half, other=sc)):
        with pytest.raises(_lib.CsError, match=r"no room for the f16 filter copy \(\d+ bytes\)") as e:
            st.similar_pairs_raw(0.9, **kw)
        assert e.value.code == _lib.CS_ERR_OOM
    monkeypatch.delenv("CS_FAULT_F16_ALLOC")
    assert st.similar_pairs_raw(0.9, scope=half, other=sc)[3] == 0  # the handle and the scopes live on
    st.close()


def test_scoped_pairs_beside_searches(VS):
    rows, _ = _planted(384)
    st = _store(VS, rows)
    ids = sorted(set(range(0, 1000, 3)) | set(PLANTED))
    sc, upper = st.scope(ids), st.scope(range(500, 1000))
    qs = synth_rows(7701, 0, 3, 384)
    want_scoped = st.similar_pairs_raw(BOUND, scope=sc, other=upper)
    want_search, want_pairs = st.search_raw(qs, 10, scope=sc), st.similar_pairs_raw(BOUND)
    assert want_scoped[3] > 60
    errors = []

    def run(call, want, name):
        try:
            for _ in range(10):
                r = call()
                if not all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(r[:3], want[:3])):
                    errors.append(name)
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=run, args=(lambda: st.similar_pairs_raw(BOUND, scope=sc, other=upper), want_scoped, "scoped")),
          threading.Thread(target=run, args=(lambda: st.search_raw(qs, 10, scope=sc), want_search, "search")),
          threading.Thread(target=run, args=(lambda: st.similar_pairs_raw(BOUND), want_pairs, "pairs"))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_src_against_vendor_with_metadata(VS):
    from codesearch_amd.vector_store import cos_to_score

    dim, n = 384, 40
    files = ["src/a.rs", "src/b.rs", "vendor/copy.rs", "lib/d.rs"]
    rows = synth_rows(7801, 0, n, dim).copy()
    paths = [files[i % len(files)] for i in range(n)]
    _plant(rows, 1, 6, 0.99)    # src/b.rs -> vendor/copy.rs: the copy
    _plant(rows, 4, 9, 0.95)    # src/a.rs -> src/b.rs: a clone inside src/
    _plant(rows, 3, 10, 0.92)   # lib/d.rs -> vendor/copy.rs
    st = VS(None, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(n))
    st.build_index()
    src, vendor = st.scope(st.chunk_ids_under("src/")), st.scope(st.chunk_ids_under("vendor/"))
    assert len(src) == 20 and len(vendor) == 10
    assert [(x.id, y.id) for x, y, _ in st.similar_pairs(0.95)] == [(1, 6), (4, 9), (3, 10)]
    across = st.similar_pairs(0.95, scope=src, other=vendor)  # score 0.95 = cosine 0.9
    assert [(x.id, y.id) for x, y, _ in across] == [(1, 6)]
    assert (across[0][0].path, across[0][1].path) == ("src/b.rs", "vendor/copy.rs") and across[0][1].content == "chunk 6"
    raw = st.similar_pairs_raw(0.9, other_files=True, scope=src, other=vendor)
    assert [np.float32(s) for _, _, s in across] == [cos_to_score(np.float32(c)) for c in raw[0]]
    assert [(x.id, y.id) for x, y, _ in st.similar_pairs(0.95, scope=vendor, other=src)] == [(1, 6)]
    inside = st.similar_pairs(0.95, scope=src)
    assert [(x.id, y.id) for x, y, _ in inside] == [(4, 9)] and inside[0][0].path == "src/a.rs"
    assert st.similar_pairs(0.999, scope=src, other=vendor) == []
    st.close()
