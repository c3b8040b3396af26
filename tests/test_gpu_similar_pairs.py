"""Similar-pairs search (cs_index_similar_pairs, codesearch_amd/csrc/scan_pairs.hip): every pair of stored chunks above a
cosine bound, exact — the corpus joined with itself on the f16 MFMA, the survivors re-scored in f32.

Ground truth comes only from code that exists without the feature: for each live chunk a, similar_raw([a ...], 1024,
exclude="self" or "file", min_cos=bound) on the streaming route, in calls of at most CS_MAX_QUERIES sources (similar_raw
splits them); the hits b > a are kept and reduced on the host by search.pairs_above.  Ids, order and total must match
exactly, cosines byte for byte.

Planted data: the background is synth_rows (no background pair at 1,000 x 384 exceeds 0.22); a pair at a target cosine c is
rows[b] = |rows[b]| (c u + sqrt(1 - c^2) w) with u the unit rows[a] and w the unit part of rows[b] orthogonal to it, computed
in float64 (within 2e-9 of the target before the rounding to f32), each b used once."""
import ctypes
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import NO_GROUP, pairs_above
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
BOUND = np.float32(0.9)


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


HUB, SPOKES = 600, [601, 602, 603, 604, 605, 640, 641, 642, 643, 644, 645]  # one tile edge (639 | 640) inside the clique
TWINS = [990, 991, 992]                                                     # identical rows, ungrouped
# where a pair near the bound sits: inside one tile; across the 127 | 128 tile edge; in tiles 0 and 7 (rows 0 and 999); on
# the diagonal (ragged, last) tile
SPOTS = [(10, 20), (127, 128), (0, 999), (900, 950)]
DELTAS = [2e-4, -2e-4, 5e-4, -5e-4]  # all inside the f16 filter's margin (1e-3): only the refine can tell them apart


def _planted(dim, rot=0, n=1000):
    """-> (rows, near): `near` = the four pairs around the bound as (a, b, delta); rot moves the deltas over the spots."""
    rows = synth_rows(7100 + dim, 0, n, dim).copy()
    near = []
    for s, (a, b) in enumerate(SPOTS):
        d = DELTAS[(s + rot) % 4]
        _plant(rows, a, b, float(BOUND) + d)
        near.append((a, b, d))
    for b in SPOKES:
        _plant(rows, HUB, b, 0.97)  # mutual cosines ~ 0.97^2 = 0.94: 66 pairs among the twelve rows
    rows[TWINS[1]] = rows[TWINS[0]]
    rows[TWINS[2]] = rows[TWINS[0]]
    return rows, near


def _files_of_8(n, ungrouped, base=0):
    """ids in files of 8 consecutive ids; the last `ungrouped` ids carry no group."""
    return {base + r: r // 8 for r in range(n - ungrouped)}


def _lookup(groups):
    return lambda ids: [groups.get(int(i), NO_GROUP) for i in ids]


def _truth(st, live_ids, bound, other):
    """{a: (cos, ids)} from the similar-chunk search on the streaming route, one source per live chunk."""
    live_ids = [int(i) for i in live_ids]
    cos, hit, cnt = st.similar_raw(live_ids, 1024, exclude="file" if other else "self", min_cos=bound)
    assert (cnt < 1024).all() or len(live_ids) <= 1025  # no list was cut
    return {a: (cos[q][:cnt[q]].copy(), hit[q][:cnt[q]].copy()) for q, a in enumerate(live_ids)}


def _check(st, live_ids, look, bound, other, max_pairs=65536):
    """similar_pairs_raw against the reduced truth, bit for bit; -> (cos, a, b, total)."""
    want = pairs_above(_truth(st, live_ids, bound, other), look, "other_group" if other else "all", bound, max_pairs)
    cos, a, b, total = st.similar_pairs_raw(bound, other_files=other, max_pairs=max_pairs)
    assert total == want[3], (total, want[3])
    assert len(a) == len(b) == len(cos) == min(total, max_pairs)
    assert a.tolist() == want[1] and b.tolist() == want[2]
    assert cos.tobytes() == np.asarray(want[0], np.float32).tobytes()
    assert (a < b).all()
    info = st.similar_pairs_info()
    assert info["candidates"] >= total and (info["bands"] >= 1 or len(live_ids) < 2)
    return cos, a, b, total


@pytest.mark.parametrize("dim,rot", [(384, 0), (768, 1), (1024, 2)])
def test_planted_pairs_around_the_bound(VS, dim, rot):
    n = 1000
    rows, near = _planted(dim, rot)
    st = _store(VS, rows)
    groups = _files_of_8(n, 40)
    live = range(n)
    # no group assigned: OTHER_GROUP is ALL
    x, y = st.similar_pairs_raw(BOUND, other_files=True), st.similar_pairs_raw(BOUND, other_files=False)
    assert all(np.asarray(p).tobytes() == np.asarray(q).tobytes() for p, q in zip(x[:3], y[:3])) and x[3] == y[3]
    st.set_groups(list(groups), list(groups.values()))
    cos, a, b, total = _check(st, live, _lookup(groups), BOUND, False)
    assert total == 71  # 66 in the clique, 3 among the identical rows, the two planted above the bound
    got = set(zip(a.tolist(), b.tolist()))
    for pa, pb, d in near:  # the refine, not the filter, decided these
        assert ((pa, pb) in got) == (d > 0), (pa, pb, d)
    assert st.similar_pairs_info()["candidates"] >= 73  # ... and the two just under the bound were candidates
    # the identical rows: three pairs with the same cosine bits, ordered by a then b, in front of everything
    assert list(zip(a[:3].tolist(), b[:3].tolist())) == [(990, 991), (990, 992), (991, 992)]
    assert cos[0].tobytes() == cos[1].tobytes() == cos[2].tobytes()
    # OTHER_GROUP: the clique loses the pairs inside files 75 (600..605) and 80 (640..645); two ungrouped rows are never a file
    cos, a, b, total = _check(st, live, _lookup(groups), BOUND, True)
    assert total == 71 - 15 - 15
    assert all(groups.get(i, -1) != groups.get(j, -2) for i, j in zip(a.tolist(), b.tolist()))
    assert (990, 991) in set(zip(a.tolist(), b.tolist()))
    # a lower bound: more of the background comes in, still exact
    _check(st, live, _lookup(groups), np.float32(0.15), False)
    _check(st, live, _lookup(groups), np.float32(0.15), True)
    st.close()


@pytest.mark.parametrize("n,pairs", [(300, 44_850), (129, 8_256), (128, 8_128), (2, 1)])
def test_full_joins_without_a_bound(VS, n, pairs):
    dim = 384
    st = _store(VS, synth_rows(7200 + n, 0, n, dim))
    groups = _files_of_8(n, min(n // 2, 40))
    st.set_groups(list(groups), list(groups.values()))
    for bound in (NEG_INF, None):
        cos, a, b, total = _check(st, range(n), _lookup(groups), bound, False)
        assert total == pairs and len(a) == pairs
    assert (np.diff(cos) <= 0).all()
    _check(st, range(n), _lookup(groups), NEG_INF, True)
    st.close()


def test_a_store_with_one_row_or_none_has_no_pair(VS):
    one = _store(VS, synth_rows(7301, 0, 1, 384))
    assert one.similar_pairs_raw(NEG_INF)[3] == 0 and len(one.similar_pairs_raw(NEG_INF, other_files=True)[0]) == 0
    assert one.similar_pairs_info()["bands"] == 0  # nothing was launched
    one.close()
    two = _store(VS, synth_rows(7302, 0, 2, 384))
    assert two.delete_chunks([0]) == 1
    two.build_index()
    assert two.similar_pairs_raw(NEG_INF)[3] == 0
    two.close()


def test_the_bound_is_strict(VS):
    rows, near = _planted(384)
    st = _store(VS, rows)
    pa, pb = [(a, b) for a, b, d in near if d == 2e-4][0]
    cos, hit, cnt = st.similar_raw([pa], 1024, exclude="self", min_cos=0.5)
    exact = np.float32(cos[0][hit[0][:cnt[0]].tolist().index(pb)])  # the pair's f32 cosine, from the similar-chunk search
    assert abs(float(exact) - 0.9002) < 1e-6
    at = st.similar_pairs_raw(exact)
    assert (pa, pb) not in set(zip(at[1].tolist(), at[2].tolist())) and at[3] == 70
    below = st.similar_pairs_raw(np.nextafter(exact, np.float32(-1)))
    assert (pa, pb) in set(zip(below[1].tolist(), below[2].tolist())) and below[3] == 71
    assert below[0][below[1].tolist().index(pa)].tobytes() == exact.tobytes()
    _check(st, range(1000), _lookup({}), exact, False)
    assert st.similar_pairs_raw(2.0)[3] == 0  # above every cosine
    st.close()


def test_id_base_and_deleted_rows(VS, monkeypatch):
    """id_base = 1,000, then 30 % of the rows deleted, in both states a built index can be in.  A delete un-builds the index
    (every search is then CS_ERR_NOT_BUILT, checked), so "before the rows move" is the build that keeps them where they are
    as tombstones (CS_INDEX_COMPACT_DEAD_PCT=0: never reclaim: the filter's bitmap test) and "after" the ordinary build,
    which reclaims: the rows move, the ids stay (the row -> id table)."""
    n, base = 1000, 1000
    rows, near = _planted(384)
    groups = _files_of_8(n, 40, base)
    look = _lookup(groups)
    kept = [(a, b) for a, b, d in near if d > 0]
    victim = base + kept[0][1]  # the b of a planted pair above the bound
    rng = np.random.default_rng(5)
    protect = {base + r for r in [HUB] + SPOKES + TWINS + [x for a, b, _ in near for x in (a, b)]}
    pool = [base + r for r in range(n) if base + r not in protect]
    gone = sorted(set(rng.choice(pool, (3 * n) // 10 - 1, replace=False).tolist()) | {victim})
    assert len(gone) == (3 * n) // 10
    live = [base + r for r in range(n) if base + r not in set(gone)]
    answers = []
    for reclaim in (False, True):
        if not reclaim:
            monkeypatch.setenv("CS_INDEX_COMPACT_DEAD_PCT", "0")
        else:
            monkeypatch.delenv("CS_INDEX_COMPACT_DEAD_PCT")
        st = _store(VS, rows, id_base=base)
        st.set_groups(list(groups), list(groups.values()))
        cos, a, b, total = _check(st, [base + r for r in range(n)], look, BOUND, False)  # id_base alone
        assert total == 71 and (base + kept[0][0], victim) in set(zip(a.tolist(), b.tolist())) and a.min() >= base
        assert st.delete_chunks(gone) == len(gone)
        with pytest.raises(_lib.CsError, match="Index not built"):
            st.similar_pairs_raw(BOUND)
        st.build_index()
        st.set_single_query_route(st.ROUTE_STREAM)
        assert st.stored_rows() == (n - len(gone) if reclaim else n) and len(st) == n - len(gone)
        cos, a, b, total = _check(st, live, look, BOUND, False)
        assert total == 70  # a deleted row of a planted pair takes the pair with it
        assert victim not in set(a.tolist()) | set(b.tolist())
        other = _check(st, live, look, BOUND, True)
        _check(st, live, look, np.float32(0.15), False)
        answers.append((cos.tobytes(), a.tobytes(), b.tobytes(), other[0].tobytes(), other[1].tobytes()))
        st.close()
    assert answers[0] == answers[1]  # tombstoned or reclaimed: the same pairs, the same bits


def test_truncation_keeps_the_total(VS):
    rows, _ = _planted(384)
    st = _store(VS, rows)
    full = st.similar_pairs_raw(BOUND)
    cos, a, b, total = _check(st, range(1000), _lookup({}), BOUND, False, max_pairs=10)
    assert total == 71 and len(a) == 10
    assert cos.tobytes() == full[0][:10].tobytes() and a.tobytes() == full[1][:10].tobytes() and b.tobytes() == full[2][:10].tobytes()
    one = st.similar_pairs_raw(BOUND, max_pairs=1)
    assert one[3] == 71 and (one[1][0], one[2][0]) == (990, 991)
    st.close()


def _raw(lib, h, min_cos, mode, max_pairs, a, b, cos, total):
    p = lambda x, t: x.ctypes.data_as(t) if x is not None else None
    return lib.cs_index_similar_pairs(h, min_cos, mode, max_pairs, p(a, _lib.u32p), p(b, _lib.u32p), p(cos, _lib.f32p),
                                      ctypes.byref(total) if total is not None else None)


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


def test_too_many_candidates_is_refused_and_the_handle_lives_on(VS, gpu_lib):
    n = 300
    st = _store(VS, synth_rows(7200 + n, 0, n, 384))
    o = _Out(100)
    assert _raw(gpu_lib, st.handle, NEG_INF, 0, 100, o.a, o.b, o.cos, o.total) == _lib.CS_ERR_UNSUPPORTED  # cand_cap 4,296 < 44,850
    msg = _lib.last_error()
    assert "candidate pairs" in msg and "raise min_cos, exclude groups" in msg and "raise max_pairs" in msg and "4296" in msg
    assert o.untouched()
    with pytest.raises(_lib.CsError, match="candidate pairs") as e:
        st.similar_pairs_raw(NEG_INF, max_pairs=100)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    cos, a, b, total = _check(st, range(n), _lookup({}), NEG_INF, False)  # a call that fits, on the same handle
    assert total == 44_850
    # max_pairs = 100 is enough once the bound leaves few pairs: truncated, not refused (cosines of this background < 0.25)
    cut = st.similar_pairs_raw(np.float32(0.12), max_pairs=100)
    want = [i for i, c in enumerate(cos) if c > np.float32(0.12)]
    assert cut[3] == len(want) and cut[0].tobytes() == cos[:min(100, len(want))].tobytes()
    st.close()


def test_a_file_of_near_duplicates(VS):
    """600 of 1,000 rows are near-duplicates of one row, all in one file: 179,700 pairs inside it.  OTHER_GROUP drops them
    inside the selection and succeeds with max_pairs = 2,000; ALL with the same cap is refused."""
    n, dim = 1000, 384
    rows = synth_rows(7401, 0, n, dim).copy()
    hog = np.arange(200, 800)
    rows[hog[1:]] = 0.95 * rows[200] + 0.05 * rows[hog[1:]]
    rows[900] = 0.95 * rows[200] + 0.05 * rows[900]  # one copy in another file: 600 pairs across files
    groups = {r: 1000 + r // 8 for r in range(n)}
    groups.update({int(r): 7 for r in hog})
    st = _store(VS, rows)
    st.set_groups(list(groups), list(groups.values()))
    cos, a, b, total = _check(st, range(n), _lookup(groups), BOUND, True, max_pairs=2000)
    assert total == 600 and (b == 900).all() and set(a.tolist()) == set(hog.tolist())
    assert not any(groups[i] == 7 and groups[j] == 7 for i, j in zip(a.tolist(), b.tolist()))
    with pytest.raises(_lib.CsError, match="candidate pairs") as e:
        st.similar_pairs_raw(BOUND, other_files=False, max_pairs=2000)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    st.close()


def test_repeat_and_no_trace_where_the_int8_copy_serves(VS):
    """5,000 rows: the int8 copy serves the index, which then holds no f16 copy — the call brings its own and leaves the
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
    qs = synth_rows(7502, 0, 6, dim)
    state, copies, before = st.filter_state(), st.filter_copies(), st.search_raw(qs, 10)
    first = st.similar_pairs_raw(BOUND)
    assert first[3] == 3 and list(zip(first[1].tolist(), first[2].tolist())) == [(2047, 2048), (3000, 3001), (5, 4999)]
    for _ in range(2):  # the same call three times: identical bytes
        again = st.similar_pairs_raw(BOUND)
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(first[:3], again[:3])) and again[3] == 3
    assert st.filter_state() == state and st.filter_copies() == copies
    after = st.search_raw(qs, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    st.set_single_query_route(st.ROUTE_STREAM)
    _check(st, range(n), _lookup(groups), BOUND, False)
    _check(st, range(n), _lookup(groups), BOUND, True)
    st.close()


def test_errors_and_their_order(VS, gpu_lib, monkeypatch):
    n, dim = 500, 384
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(7601, 0, n, dim))
    o = _Out(8)
    nan = float("nan")

    def fails(code, text, *args, handle=True):
        assert _raw(gpu_lib, st.handle if handle else None, *args) == code
        assert text in _lib.last_error(), _lib.last_error()
        assert o.untouched()

    bad = _lib.CS_ERR_BAD_ARG
    # 1. the handle and the built state, before everything behind them
    fails(bad, "null index handle", nan, 9, 0, None, None, None, None, handle=False)
    fails(_lib.CS_ERR_NOT_BUILT, "Index not built. Call build_index() after inserting chunks.", nan, 9, 0, None, None, None, None)
    st.build_index()
    # 2. a null output pointer, before the mode
    fails(bad, "null buffer", nan, 9, 0, None, o.b, o.cos, o.total)
    fails(bad, "null buffer", nan, 9, 0, o.a, None, o.cos, o.total)
    fails(bad, "null buffer", nan, 9, 0, o.a, o.b, None, o.total)
    fails(bad, "null buffer", nan, 9, 0, o.a, o.b, o.cos, None)
    # 3. the mode, before the bound;  4. the bound, before max_pairs;  5. max_pairs
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", nan, 2, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", nan, -1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "min_cos is NaN", nan, 1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "max_pairs must be in 1..4194304, got 0", 0.5, 1, 0, o.a, o.b, o.cos, o.total)
    fails(bad, "max_pairs must be in 1..4194304, got 4194305", 0.5, 0, _lib.CS_MAX_PAIRS + 1, o.a, o.b, o.cos, o.total)
    assert _raw(gpu_lib, st.handle, 0.5, 1, 8, o.a, o.b, o.cos, o.total) == _lib.CS_OK and o.total.value == 0
    st.close()
    # 6. a dim the f16 filter has no tiles for: max_pairs is still checked first
    odd = VS(None, 100)
    odd.insert_embeddings(synth_rows(7602, 0, 50, 100))
    odd.build_index()
    o = _Out(8)
    assert _raw(gpu_lib, odd.handle, 0.5, 0, 0, o.a, o.b, o.cos, o.total) == bad and "max_pairs must be" in _lib.last_error()
    assert _raw(gpu_lib, odd.handle, 0.5, 0, 8, o.a, o.b, o.cos, o.total) == _lib.CS_ERR_UNSUPPORTED
    assert "dim 384, 768 or 1024" in _lib.last_error() and "got 100" in _lib.last_error() and o.untouched()
    odd.close()
    # 7. no f16 copy because CS_INDEX_SPLIT=0 turned the filter copies off
    monkeypatch.setenv("CS_INDEX_SPLIT", "0")
    off = VS(None, dim)
    off.insert_embeddings(synth_rows(7603, 0, 50, dim))
    off.build_index()
    assert _raw(gpu_lib, off.handle, 0.5, 0, 8, o.a, o.b, o.cos, o.total) == _lib.CS_ERR_UNSUPPORTED
    assert "CS_INDEX_SPLIT=0" in _lib.last_error() and o.untouched()
    off.close()
    monkeypatch.delenv("CS_INDEX_SPLIT")
    # the Python layer: a sharded store has no form of the call
    sharded = VS(None, dim, devices=[0, 0])
    with pytest.raises(_lib.CsError, match="no similar-pairs search: no cs_shards_ form yet") as e:
        sharded.similar_pairs_raw(0.9)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    sharded.close()


@pytest.mark.parametrize("n", [1000, 5000])  # the index's own f16 copy (the build's) / the call's own (the int8 copy serves)
def test_no_room_for_the_f16_copy(lab_lib, VS, monkeypatch, n):
    monkeypatch.setenv("CS_FAULT_F16_ALLOC", "1")
    st = VS(None, 384)
    st.insert_embeddings(synth_rows(7604, 0, n, 384))
    st.build_index()
    with pytest.raises(_lib.CsError, match="no room for the f16 filter copy") as e:
        st.similar_pairs_raw(0.9)
    assert e.value.code == _lib.CS_ERR_OOM
    st.close()


def test_pairs_beside_searches(VS):
    rows, _ = _planted(384)
    st = _store(VS, rows)
    qs = synth_rows(7701, 0, 3, 384)
    want_pairs, want_search = st.similar_pairs_raw(BOUND), st.search_raw(qs, 10)
    errors = []

    def pairs():
        try:
            for _ in range(10):
                r = st.similar_pairs_raw(BOUND)
                if r[3] != want_pairs[3] or not all(x.tobytes() == y.tobytes() for x, y in zip(r[:3], want_pairs[:3])):
                    errors.append("pairs")
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    def search():
        try:
            for _ in range(10):
                r = st.search_raw(qs, 10)
                if not all(x.tobytes() == y.tobytes() for x, y in zip(r, want_search)):
                    errors.append("search")
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    th = [threading.Thread(target=pairs), threading.Thread(target=search), threading.Thread(target=pairs)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_similar_pairs_returns_results_with_metadata(VS):
    from codesearch_amd.vector_store import cos_to_score

    dim, n = 384, 40
    files = ["src/a.rs", "src/b.rs", "vendor/copy.rs", "lib/d.rs"]
    rows = synth_rows(7801, 0, n, dim).copy()
    paths = [files[i % len(files)] for i in range(n)]
    _plant(rows, 1, 6, 0.99)    # src/b.rs -> vendor/copy.rs: a copy in another file
    _plant(rows, 4, 8, 0.95)    # src/a.rs -> src/a.rs: a clone inside one file
    _plant(rows, 3, 10, 0.92)   # lib/d.rs -> vendor/copy.rs
    st = VS(None, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(n))
    st.build_index()
    across = st.similar_pairs(0.95)  # score 0.95 = cosine 0.9
    assert [(x.id, y.id) for x, y, _ in across] == [(1, 6), (3, 10)]
    assert [(x.path, y.path) for x, y, _ in across] == [("src/b.rs", "vendor/copy.rs"), ("lib/d.rs", "vendor/copy.rs")]
    raw = st.similar_pairs_raw(0.9, other_files=True)
    assert [np.float32(s) for _, _, s in across] == [cos_to_score(np.float32(c)) for c in raw[0]]
    every = st.similar_pairs(0.95, other_files=False)
    assert [(x.id, y.id) for x, y, _ in every] == [(1, 6), (4, 8), (3, 10)]
    assert every[1][0].content == "chunk 4" and every[1][1].content == "chunk 8"
    assert st.similar_pairs(0.999) == []
    assert len(st.similar_pairs(0.95, other_files=False, max_pairs=2)) == 2
    st.close()
