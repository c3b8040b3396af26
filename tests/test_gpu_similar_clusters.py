"""Similar-clusters search (cs_index_similar_clusters, codesearch_amd/csrc/scan_clusters.hip): the clone classes of the
store — the connected components of the graph whose edges are the pairs cs_index_similar_pairs would count — as one label
per id, the smallest id of the class.

The oracle is code that exists without the feature: similar_pairs_raw(bound, mode, max_pairs = 1 << 20) on the same store,
reduced on the host by search.clusters_of_pairs.  The oracle call must be neither refused nor cut, so oracle stores hold at
most 1,000 rows (499,500 pairs against a candidate bound of 2,101,248) or few pairs, and the helper asserts total <=
max_pairs.  Labels must match exactly.  Two tests know their components by construction and need no pairs kernel at all.

Planted data as in test_gpu_similar_pairs.py: the background is synth_rows (no background pair at 1,000 x 384 exceeds
0.25); a pair at a target cosine c is rows[b] = |rows[b]| (c u + sqrt(1 - c^2) w), computed in float64."""
import ctypes
import os
import subprocess
import threading

import numpy as np
import pytest

from codesearch_amd import _lib
from codesearch_amd.search import clusters_of_pairs
from codesearch_amd.synth import synth_rows

pytestmark = pytest.mark.gpu

NO_ID = _lib.CS_NO_ID
BOUND = np.float32(0.9)
ORACLE_PAIRS = 1 << 20
MARGIN = 1.02e-3  # filter_margin(384) where the f16 MFMA takes subnormal inputs exactly (scan_filter.hip's header)


@pytest.fixture(scope="module")
def VS(gpu_lib):
    from codesearch_amd import VectorStore

    assert gpu_lib.cs_device_count() >= 1, "no HIP device visible"
    return VectorStore


def _store(VS, rows, id_base=0, groups=None):
    st = VS(None, rows.shape[1], id_base=id_base)
    st.insert_embeddings(rows)
    st.build_index()
    if groups:
        st.set_groups(list(groups), list(groups.values()))
    return st


def _plant(rows, a, b, c):
    u = rows[a].astype(np.float64)
    u /= np.linalg.norm(u)
    x = rows[b].astype(np.float64)
    w = x - (x @ u) * u
    w /= np.linalg.norm(w)
    rows[b] = (np.linalg.norm(x) * (c * u + np.sqrt(1.0 - c * c) * w)).astype(np.float32)


def _files_of_8(n, base=0):
    return {base + r: r // 8 for r in range(n)}


def _oracle(st, live_ids, bound, other):
    """-> ({id: label}, clusters, members) from the pairs call, neither refused nor cut."""
    cos, a, b, total = st.similar_pairs_raw(bound, other_files=other, max_pairs=ORACLE_PAIRS)
    assert total <= ORACLE_PAIRS and len(a) == len(b) == total, "the oracle's pair list was cut"
    return clusters_of_pairs(live_ids, a, b), total


def _expected(labels_by_id, n_labels, id_base):
    want = np.full(n_labels, NO_ID, np.uint32)
    for i, lab in labels_by_id.items():
        want[i - id_base] = lab
    return want


def _check(st, live_ids, bound, other, id_base=0):
    """similar_clusters_raw against the reduced oracle, exactly; -> (labels, clusters, members, the oracle's pair count)."""
    (want, wc, wm), total = _oracle(st, live_ids, bound, other)
    labels, clusters, members = st.similar_clusters_raw(bound, other_files=other)
    assert labels.dtype == np.uint32 and len(labels) == st.next_id() - id_base
    expect = _expected(want, len(labels), id_base)
    diff = np.flatnonzero(labels != expect)
    assert diff.size == 0, (diff[:8], labels[diff[:8]], expect[diff[:8]])
    assert (clusters, members) == (wc, wm)
    return labels, clusters, members, total


def _random_rows(n, dim):
    """synth_rows with a few planted clones where there is room: a pair across the store, a neighbour pair, a chain of
    three over a tile edge."""
    rows = synth_rows(8100 + n + dim, 0, n, dim).copy()
    if n >= 200:
        _plant(rows, 0, n - 1, 0.95)
        _plant(rows, 9, 10, 0.97)
        _plant(rows, 127, 128, 0.96)
        _plant(rows, 128, 140, 0.96)
    return rows


@pytest.mark.parametrize("n,dim", [(2, 384), (128, 384), (129, 384), (300, 384), (1000, 384), (300, 768), (300, 1024)])
def test_random_graphs_against_the_oracle(VS, n, dim):
    st = _store(VS, _random_rows(n, dim), groups=_files_of_8(n))
    live = range(n)
    for bound in (np.float32(0.12), BOUND):
        for other in (False, True):
            labels, clusters, members, total = _check(st, live, bound, other)
            print(f"n={n} dim={dim} bound={bound} other={other}: {total} pairs, {clusters} classes, {members} members")
    if n >= 200:
        labels = st.similar_clusters_raw(BOUND)[0]
        assert labels[n - 1] == 0 and labels[10] == 9 and labels[128] == 127 and labels[140] == 127
        assert st.similar_clusters_raw(BOUND)[1:] == (3, 7)
        # 9 and 10 are one file: in OTHER_GROUP that edge is none
        assert st.similar_clusters_raw(BOUND, other_files=True)[0][10] == 10
    # no bound at all: everything is one class (every cosine is finite and above -inf)
    labels, clusters, members = st.similar_clusters_raw(None)
    assert (labels == 0).all() and (clusters, members) == (1, n)
    assert st.similar_clusters_raw(2.0)[1:] == (0, 0)  # above every cosine: everybody alone
    assert st.similar_clusters_raw(2.0)[0].tolist() == list(range(n))
    st.close()


def test_small_stores_launch_nothing(VS):
    one = _store(VS, synth_rows(8201, 0, 1, 384))
    labels, clusters, members = one.similar_clusters_raw(-1.0)
    assert labels.tolist() == [0] and (clusters, members) == (0, 0)
    assert one.similar_clusters_info()["launches"] == 0
    one.close()
    two = _store(VS, synth_rows(8202, 0, 2, 384), id_base=50)
    assert two.similar_clusters_raw(-1.0)[0].tolist() == [50, 50]
    assert two.similar_clusters_info()["launches"] >= 1
    assert two.delete_chunks([50]) == 1
    two.build_index()
    labels, clusters, members = two.similar_clusters_raw(-1.0)
    assert labels.tolist() == [NO_ID, 51] and (clusters, members) == (0, 0)
    assert two.similar_clusters_info() == {"tile_pairs_scored": 0, "tile_pairs_skipped": 0, "rescored_pairs": 0, "launches": 0,
                                           "join_ms": 0.0, "label_ms": 0.0}
    two.close()


def _chain(n, dim):
    rows = np.zeros((n, dim), np.float32)
    for i in range(n):
        rows[i, i] = rows[i, i + 1] = np.float32(np.sqrt(0.5))
    return rows


def test_a_chain_is_one_component_and_a_deleted_link_cuts_it(VS):
    """x_i = normalize(e_i + e_(i+1)), i < 300: neighbours have cosine 0.5, every other pair 0 — the only edges at bound 0.4
    join neighbours, so the components are known without any pairs kernel: one chain across three tiles."""
    n = 300
    st = _store(VS, _chain(n, 384))
    labels, clusters, members = st.similar_clusters_raw(0.4)
    assert (labels == 0).all() and (clusters, members) == (1, n)
    assert st.similar_clusters_raw(0.6)[0].tolist() == list(range(n))  # above the neighbours' cosine: nobody
    _check(st, range(n), np.float32(0.4), False)
    assert st.delete_chunks([150]) == 1
    st.build_index()
    labels, clusters, members = st.similar_clusters_raw(0.4)
    assert (labels[:150] == 0).all() and labels[150] == NO_ID and (labels[151:] == 151).all()
    assert (clusters, members) == (2, n - 1)
    st.close()


# where a pair near the bound sits: inside one tile; across the 127 | 128 tile edge; in tiles 0 and 7 (rows 0 and 999); on
# the diagonal (ragged, last) tile; and four more for the far side of the margin
SPOTS = [(10, 20), (127, 128), (0, 999), (900, 950), (300, 310), (383, 384), (5, 700), (960, 990)]
DELTAS = [MARGIN / 2, -MARGIN / 2, 2 * MARGIN, -2 * MARGIN, -MARGIN / 2, MARGIN / 2, -2 * MARGIN, 2 * MARGIN]
HUB, SPOKES = 600, [601, 602, 603, 604, 605, 640, 641, 642, 643, 644, 645]
TWINS = [990 - 20, 991 - 20, 992 - 20]  # identical rows


def _planted(dim=384, n=1000):
    rows = synth_rows(8300 + dim, 0, n, dim).copy()
    for (a, b), d in zip(SPOTS, DELTAS):
        _plant(rows, a, b, float(BOUND) + d)
    for b in SPOKES:
        _plant(rows, HUB, b, 0.97)
    rows[TWINS[1]] = rows[TWINS[0]]
    rows[TWINS[2]] = rows[TWINS[0]]
    return rows


@pytest.fixture(scope="module")
def planted_store(VS):
    st = _store(VS, _planted(), groups=_files_of_8(1000))
    yield st
    st.close()


def test_planted_pairs_around_the_bound(planted_store):
    """Planted pairs at the bound +- margin / 2 (the rescore decides them) and +- 2 margin (above: united without a rescore;
    below: ruled out by the f16 product): exactly the pairs planted above the bound are classes."""
    st = planted_store
    labels, clusters, members, total = _check(st, range(1000), BOUND, False)
    for (a, b), d in zip(SPOTS, DELTAS):
        assert (labels[b] == a) == (d > 0), (a, b, d)
        assert labels[a] == a
    assert (labels[SPOKES] == HUB).all() and (labels[TWINS] == TWINS[0]).all()
    assert (clusters, members) == (4 + 1 + 1, 8 + 12 + 3)
    assert st.similar_clusters_info()["rescored_pairs"] >= 4  # the four at +- margin / 2 at least
    # OTHER_GROUP: 600..605 and 640..645 are one file each and stay one class through the hub's edges across files
    labels, clusters, members, total = _check(st, range(1000), BOUND, True)
    assert (labels[SPOKES[5:]] == HUB).all()
    _check(st, range(1000), np.float32(0.15), False)
    _check(st, range(1000), np.float32(0.15), True)


def test_the_bound_is_strict_at_equal_bits(planted_store):
    st = planted_store
    pa, pb = SPOTS[0]  # planted at the bound + margin / 2
    cos, a, b, total = st.similar_pairs_raw(np.float32(0.85), max_pairs=ORACLE_PAIRS)
    exact = np.float32(cos[[i for i in range(total) if (a[i], b[i]) == (pa, pb)][0]])  # the pair's f32 cosine
    assert abs(float(exact) - (0.9 + MARGIN / 2)) < 1e-6
    assert st.similar_clusters_raw(exact)[0][pb] == pb  # equal bits: no edge
    assert st.similar_clusters_raw(np.nextafter(exact, np.float32(-1)))[0][pb] == pa  # one ulp under the cosine
    assert st.similar_clusters_raw(np.nextafter(exact, np.float32(2)))[0][pb] == pb
    for bound in (exact, np.nextafter(exact, np.float32(-1))):
        _check(st, range(1000), bound, False)


def _equi_cosine(n=380, dim=384, c=0.9):
    """x_i = sqrt(c) u + sqrt(1 - c) e_i with u a unit vector over the last four coordinates: every pair has cosine c in
    exact arithmetic, and the f32 rounding of rows and scan puts each on one side of the f32 bound."""
    u = np.zeros(dim)
    u[n:] = np.array([0.5, -0.3, 0.7, 0.41])[:dim - n]
    u /= np.linalg.norm(u)
    rows = np.sqrt(c) * np.tile(u, (n, 1))
    rows[np.arange(n), np.arange(n)] = np.sqrt(1 - c)
    scale = 1.0 + 0.37 * (np.arange(n) % 7)[:, None]  # magnitudes differ: the unit rows' roundings do too
    return (rows * scale).astype(np.float32)


@pytest.fixture(scope="module")
def equi_rows():
    return _equi_cosine()


def test_an_equi_cosine_set_is_all_ambiguous(VS, equi_rows):
    """380 rows, every one of the 72,010 pairs at the bound itself: none can be decided by the f16 product, all go through
    the buffer and the rescore, and f32 rounding puts some on each side.  Labels equal the oracle's exactly."""
    st = _store(VS, equi_rows)
    labels, clusters, members, total = _check(st, range(380), BOUND, False)
    print(f"equi-cosine: {total} of 72010 pairs above the bound, {clusters} classes, {members} members")
    assert 0 < total < 72010, "the set no longer straddles the bound: the test's data needs another look"
    info = st.similar_clusters_info()
    assert info["rescored_pairs"] > 0 and info["tile_pairs_scored"] + info["tile_pairs_skipped"] == 6
    first = st.similar_clusters_raw(BOUND)
    for _ in range(2):  # three calls: identical bytes
        again = st.similar_clusters_raw(BOUND)
        assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:]
    st.close()


def _hog_rows():
    n, dim = 1000, 384
    rows = synth_rows(7401, 0, n, dim).copy()
    hog = np.arange(200, 800)
    rows[hog[1:]] = 0.95 * rows[200] + 0.05 * rows[hog[1:]]
    rows[900] = 0.95 * rows[200] + 0.05 * rows[900]  # one copy in another file
    groups = {r: 1000 + r // 8 for r in range(n)}
    groups.update({int(r): 7 for r in hog})
    return rows, hog, groups


def test_a_file_of_near_duplicates_is_one_class_not_a_refusal(VS):
    rows, hog, groups = _hog_rows()
    st = _store(VS, rows, groups=groups)
    with pytest.raises(_lib.CsError, match="candidate pairs") as e:
        st.similar_pairs_raw(BOUND, other_files=False, max_pairs=2000)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    labels, clusters, members, total = _check(st, range(1000), BOUND, False)
    assert total == 180_300
    assert (labels[hog] == 200).all() and labels[900] == 200 and (clusters, members) == (1, 601)
    rest = np.setdiff1d(np.arange(1000), np.append(hog, 900))
    assert (labels[rest] == rest).all()
    first = st.similar_clusters_raw(BOUND)
    for _ in range(2):  # three calls: identical bytes, however the unions raced
        again = st.similar_clusters_raw(BOUND)
        assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:]
    # OTHER_GROUP: no edge inside the file, and still one class through the copy in the other file
    labels, clusters, members, total = _check(st, range(1000), BOUND, True)
    assert total == 600 and (labels[hog] == 200).all() and labels[900] == 200 and (clusters, members) == (1, 601)
    # without the copy the 600 are alone
    assert st.delete_chunks([900]) == 1
    st.build_index()
    live = [i for i in range(1000) if i != 900]
    labels, clusters, members, total = _check(st, live, BOUND, True)
    assert total == 0 and (labels[hog] == hog).all() and labels[900] == NO_ID and (clusters, members) == (0, 0)
    labels, clusters, members, total = _check(st, live, BOUND, False)
    assert (labels[hog] == 200).all() and (clusters, members) == (1, 600)
    st.close()


def test_id_base_deleted_rows_and_a_reclaiming_build(VS, monkeypatch):
    """id_base = 1,000 and 30 % of the rows deleted — the smallest member of two classes among them — in both states a
    built index can be in: tombstones kept (CS_INDEX_COMPACT_DEAD_PCT=0) and reclaimed (rows move, ids stay)."""
    n, base = 1000, 1000
    rows = _planted()
    groups = _files_of_8(n, base)
    rng = np.random.default_rng(11)
    protect = set(SPOKES + TWINS[1:] + [x for p in SPOTS for x in p])
    pool = [r for r in range(n) if r not in protect and r not in (HUB, TWINS[0])]
    gone_rows = sorted(set(rng.choice(pool, (3 * n) // 10 - 2, replace=False).tolist()) | {HUB, TWINS[0]})
    gone = [base + r for r in gone_rows]
    live = [base + r for r in range(n) if r not in set(gone_rows)]
    answers = []
    for reclaim in (False, True):
        if not reclaim:
            monkeypatch.setenv("CS_INDEX_COMPACT_DEAD_PCT", "0")
        else:
            monkeypatch.delenv("CS_INDEX_COMPACT_DEAD_PCT")
        st = _store(VS, rows, id_base=base, groups=groups)
        labels = _check(st, [base + r for r in range(n)], BOUND, False, id_base=base)[0]  # id_base alone
        assert (labels[SPOKES] == base + HUB).all() and labels.min() >= base
        assert st.delete_chunks(gone) == len(gone)
        with pytest.raises(_lib.CsError, match="Index not built"):
            st.similar_clusters_raw(BOUND)
        st.build_index()
        assert st.stored_rows() == (n - len(gone) if reclaim else n) and len(st) == n - len(gone)
        labels, clusters, members, total = _check(st, live, BOUND, False, id_base=base)
        assert (labels[gone_rows] == NO_ID).all() and (labels != NO_ID).sum() == len(live)
        # the hub is gone: the spokes are still clones of each other (0.97^2), labelled by the smallest of them
        assert (labels[SPOKES] == base + SPOKES[0]).all()
        assert labels[TWINS[1]] == labels[TWINS[2]] == base + TWINS[1]
        other = _check(st, live, BOUND, True, id_base=base)
        _check(st, live, np.float32(0.15), False, id_base=base)
        # n_labels is the ids issued, not the rows stored or live: off by one either way is refused, nothing written
        for wrong in (n - 1, n + 1, len(live)):
            buf = np.full(n + 1, 0xA5A5A5A5, np.uint32)
            rc = st._lib.cs_index_similar_clusters(st.handle, 0.9, 0, buf.ctypes.data_as(_lib.u32p), wrong, None, None)
            assert rc == _lib.CS_ERR_BAD_ARG and str(n) in _lib.last_error() and str(wrong) in _lib.last_error()
            assert "n_labels" in _lib.last_error() and (buf == 0xA5A5A5A5).all()
        answers.append((labels.tobytes(), clusters, members, other[0].tobytes()))
        st.close()
    assert answers[0] == answers[1]  # tombstoned or reclaimed: the same labels


def test_many_launches_and_an_overflowing_buffer_change_nothing(lab_lib, VS, monkeypatch, equi_rows):
    """Two laboratory knobs (the diagnostic library reads them) reach the paths a small store never takes by itself: a launch
    of two tile pairs, and the ambiguous buffer at its minimum of one tile pair's worth — the equi-cosine set's first launch
    then holds 8,128 + 16,384 ambiguous pairs and is split."""
    rows, hog, groups = _hog_rows()
    stores = [_store(VS, equi_rows), _store(VS, rows, groups=groups)]
    default = [(st.similar_clusters_raw(BOUND), st.similar_clusters_raw(BOUND, other_files=True)) for st in stores]
    stores[0].similar_clusters_raw(BOUND)
    assert stores[0].similar_clusters_info()["launches"] == 2  # 3 tiles: the first tile row, then the rest
    monkeypatch.setenv("CS_CLUSTERS_LAUNCH_TILE_PAIRS", "2")
    monkeypatch.setenv("CS_CLUSTERS_AMBIGUOUS_CAP", "1")
    for st, want, tile_pairs in zip(stores, default, (6, 36)):
        for other in (False, True):
            got = st.similar_clusters_raw(BOUND, other_files=other)
            assert got[0].tobytes() == want[other][0].tobytes() and got[1:] == want[other][1:]
            info = st.similar_clusters_info()
            print(info)
            assert info["launches"] > 1
            assert info["tile_pairs_scored"] + info["tile_pairs_skipped"] == tile_pairs
    # the equi-cosine set: launches (0,0)+(0,1) overflowed and were repeated as halves: more launches than 6 / 2
    stores[0].similar_clusters_raw(BOUND)
    assert stores[0].similar_clusters_info()["launches"] > 3
    # the hog in ALL: tiles 2..5 hold nothing but the file, and are one class after their first tile row
    stores[1].similar_clusters_raw(BOUND)
    assert stores[1].similar_clusters_info()["tile_pairs_skipped"] > 0
    for st in stores:
        st.close()


def test_no_trace_where_the_int8_copy_serves(VS):
    """5,000 rows: the int8 copy serves the index, which then holds no f16 copy — the call brings its own and leaves the
    index as it was: the same filter state and copies, the same bits from a search on the default route."""
    n, dim = 5000, 384
    rows = synth_rows(7501, 0, n, dim).copy()
    spots = [(5, 4999), (127, 128), (3000, 3001), (4990, 4995), (2047, 2048), (128, 4000)]
    for i, (a, b) in enumerate(spots):
        _plant(rows, a, b, 0.9 + [2e-4, -2e-4, 5e-4, -5e-4, 0.05, 0.03][i])
    st = _store(VS, rows, groups=_files_of_8(n))
    assert st.filter_state()[0] == 2 and st.filter_copies()[:2] == (True, False)
    qs = synth_rows(7502, 0, 6, dim)
    state, copies, before = st.filter_state(), st.filter_copies(), st.search_raw(qs, 10)
    first = st.similar_clusters_raw(BOUND)
    assert first[1:] == (4, 8) and first[0][4999] == 5 and first[0][3001] == 3000 and first[0][2048] == 2047
    assert first[0][4000] == 128  # 127 ~ 128 was planted under the bound, 128 ~ 4000 above
    assert first[0][128] == 128 and first[0][4995] == 4995
    for _ in range(2):
        again = st.similar_clusters_raw(BOUND)
        assert again[0].tobytes() == first[0].tobytes() and again[1:] == first[1:]
    assert st.filter_state() == state and st.filter_copies() == copies
    after = st.search_raw(qs, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    _check(st, range(n), BOUND, False)  # few pairs: the oracle call is neither refused nor cut (asserted)
    _check(st, range(n), BOUND, True)
    st.close()


def test_clusters_beside_searches(planted_store):
    st = planted_store
    qs = synth_rows(7701, 0, 3, 384)
    want, want_search = st.similar_clusters_raw(BOUND), st.search_raw(qs, 10)
    errors = []

    def clusters():
        try:
            for _ in range(10):
                r = st.similar_clusters_raw(BOUND)
                if r[0].tobytes() != want[0].tobytes() or r[1:] != want[1:]:
                    errors.append("clusters")
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

    th = [threading.Thread(target=clusters), threading.Thread(target=search), threading.Thread(target=clusters)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors


class _Out:
    """Output buffers prefilled with a pattern: a failing call writes nothing."""

    def __init__(self, room):
        self.labels = np.full(room, 0xA5A5A5A5, np.uint32)
        self.clusters = ctypes.c_uint64(0x7777)
        self.members = ctypes.c_uint64(0x8888)

    def untouched(self):
        return (self.labels == 0xA5A5A5A5).all() and self.clusters.value == 0x7777 and self.members.value == 0x8888


def _raw(lib, h, min_cos, mode, o, n_labels, labels=True):
    return lib.cs_index_similar_clusters(h, min_cos, mode, o.labels.ctypes.data_as(_lib.u32p) if labels else None, n_labels,
                                         ctypes.byref(o.clusters), ctypes.byref(o.members))


def test_errors_and_their_order(VS, gpu_lib, monkeypatch):
    n, dim = 500, 384
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(7601, 0, n, dim))
    o = _Out(n + 8)
    nan = float("nan")

    def fails(code, text, *args, handle=True, **kw):
        assert _raw(gpu_lib, st.handle if handle else None, *args, **kw) == code
        assert text in _lib.last_error(), _lib.last_error()
        assert o.untouched()

    bad = _lib.CS_ERR_BAD_ARG
    # 1. the handle and the built state, before everything behind them
    fails(bad, "null index handle", nan, 9, o, n + 1, handle=False, labels=False)
    fails(_lib.CS_ERR_NOT_BUILT, "Index not built. Call build_index() after inserting chunks.", nan, 9, o, n + 1, labels=False)
    st.build_index()
    # 2. a null out_label, before the mode;  3. the mode, before the bound;  4. the bound, before n_labels;  5. n_labels
    fails(bad, "null buffer", nan, 9, o, n + 1, labels=False)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", nan, 2, o, n + 1)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", nan, -1, o, n + 1)
    fails(bad, "min_cos is NaN", nan, 1, o, n + 1)
    fails(bad, f"= {n} ", 0.5, 1, o, n + 1)
    fails(bad, f"= {n} ", 0.5, 0, o, 0)
    assert _raw(gpu_lib, st.handle, 0.5, 1, o, n) == _lib.CS_OK and (o.clusters.value, o.members.value) == (0, 0)
    assert o.labels[:n].tolist() == list(range(n)) and (o.labels[n:] == 0xA5A5A5A5).all()  # nothing past n_labels
    # the counts are optional
    assert gpu_lib.cs_index_similar_clusters(st.handle, 0.5, 0, o.labels.ctypes.data_as(_lib.u32p), n, None, None) == _lib.CS_OK
    st.close()
    # 6. a dim the f16 filter has no tiles for: n_labels is still checked first
    odd = VS(None, 100)
    odd.insert_embeddings(synth_rows(7602, 0, 50, 100))
    odd.build_index()
    o = _Out(64)
    assert _raw(gpu_lib, odd.handle, 0.5, 0, o, 49) == bad and "n_labels" in _lib.last_error() and o.untouched()
    assert _raw(gpu_lib, odd.handle, 0.5, 0, o, 50) == _lib.CS_ERR_UNSUPPORTED
    assert "dim 384, 768 or 1024" in _lib.last_error() and "got 100" in _lib.last_error() and o.untouched()
    odd.close()
    # 7. no f16 copy because CS_INDEX_SPLIT=0 turned the filter copies off
    monkeypatch.setenv("CS_INDEX_SPLIT", "0")
    off = VS(None, dim)
    off.insert_embeddings(synth_rows(7603, 0, 50, dim))
    off.build_index()
    assert _raw(gpu_lib, off.handle, 0.5, 0, o, 50) == _lib.CS_ERR_UNSUPPORTED
    assert "CS_INDEX_SPLIT=0" in _lib.last_error() and o.untouched()
    off.close()
    monkeypatch.delenv("CS_INDEX_SPLIT")
    # the Python layer: a sharded store has no form of the call
    sharded = VS(None, dim, devices=[0, 0])
    with pytest.raises(_lib.CsError, match="no similar-clusters search: no cs_shards_ form yet") as e:
        sharded.similar_clusters_raw(0.9)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    with pytest.raises(_lib.CsError, match="no similar-clusters search"):
        sharded.similar_clusters(0.95)
    sharded.close()


@pytest.mark.parametrize("n", [1000, 5000])  # the index's own f16 copy (the build's) / the call's own (the int8 copy serves)
def test_no_room_for_the_f16_copy(lab_lib, VS, monkeypatch, n):
    monkeypatch.setenv("CS_FAULT_F16_ALLOC", "1")
    st = VS(None, 384)
    st.insert_embeddings(synth_rows(7604, 0, n, 384))
    st.build_index()
    with pytest.raises(_lib.CsError, match="no room for the f16 filter copy") as e:
        st.similar_clusters_raw(0.9)
    assert e.value.code == _lib.CS_ERR_OOM
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_similar_clusters_returns_classes_with_metadata(VS):
    dim, n = 384, 40
    files = ["src/a.rs", "src/b.rs", "vendor/copy.rs", "lib/d.rs"]
    rows = synth_rows(7801, 0, n, dim).copy()
    paths = [files[i % len(files)] for i in range(n)]
    _plant(rows, 1, 6, 0.99)    # src/b.rs -> vendor/copy.rs
    _plant(rows, 6, 13, 0.99)   # vendor/copy.rs -> src/b.rs: 1, 6, 13 are one class; 1 and 13 share a file
    _plant(rows, 4, 8, 0.95)    # src/a.rs -> src/a.rs: a clone inside one file
    _plant(rows, 3, 10, 0.92)   # lib/d.rs -> vendor/copy.rs
    st = VS(None, dim)
    assert st.insert_chunks_with_ids(_file_chunks(rows, paths)) == list(range(n))
    st.build_index()
    across = st.similar_clusters(0.95)  # score 0.95 = cosine 0.9; other_files by default
    assert [[r.id for r in c] for c in across] == [[1, 6, 13], [3, 10]]
    assert [r.path for r in across[0]] == ["src/b.rs", "vendor/copy.rs", "src/b.rs"]
    assert across[1][1].content == "chunk 10"
    every = st.similar_clusters(0.95, other_files=False)
    assert [[r.id for r in c] for c in every] == [[1, 6, 13], [3, 10], [4, 8]]  # largest first, then by label
    assert [[r.id for r in c] for c in st.similar_clusters(0.95, other_files=False, min_size=3)] == [[1, 6, 13]]
    alone = st.similar_clusters(0.95, other_files=False, min_size=1)
    assert len(alone) == n - 7 + 3 and [len(c) for c in alone[:4]] == [3, 2, 2, 1] and alone[3][0].id == 0
    assert st.similar_clusters(0.9999) == []
    # a chunk without metadata is skipped, and the class is sized by what remains
    del st._meta[10]
    assert [[r.id for r in c] for c in st.similar_clusters(0.95)] == [[1, 6, 13]]
    st.close()


def test_cpp_wrapper_reports_clone_classes():
    """host/codesearch_gpu.hpp: VectorStore::similar_clusters (tests/cpp/similar_clusters_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "similar_clusters_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "similar_clusters_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "similar clusters host ok" in r.stdout
