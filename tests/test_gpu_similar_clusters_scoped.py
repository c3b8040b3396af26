"""Scoped similar-clusters search (cs_index_similar_clusters_scoped, codesearch_amd/csrc/scan_clusters_scoped.hip): the clone
classes inside one scope or between two — the connected components of the graph whose vertices are the live ids of A u B
and whose edges are the pairs cs_index_similar_pairs_scoped would count — as (id, label) per vertex, the label the smallest
id of the class.

The oracle everywhere is code that exists without the feature: similar_pairs_raw(bound, other_files, max_pairs = 1 << 20,
scope=, other=) reduced by search.clusters_of_pairs over the live ids of A u B.  The helper asserts total <= max_pairs, so the
oracle call was neither refused nor cut: every oracle store holds at most 1,000 rows, and 1,000 rows hold 499,500 pairs,
under 1 << 20 (the 5,000-row store of the no-trace test holds a handful of pairs above its bound, asserted likewise).
Labels, ids, out_n and both counts must match exactly.  Two tests know their components by construction.

Planted data as in test_gpu_similar_clusters.py (restated here): the background is synth_rows (no background pair at 1,000 x
384 exceeds 0.25); a pair at a target cosine c is rows[b] = |rows[b]| (c u + sqrt(1 - c^2) w), computed in float64."""
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


def _oracle(st, sa, sb, vertices, bound, other):
    """-> (({id: label}, clusters, members), the pair count) from the scoped pairs call, neither refused nor cut."""
    cos, a, b, total = st.similar_pairs_raw(bound, other_files=other, max_pairs=ORACLE_PAIRS, scope=sa, other=sb)
    assert total <= ORACLE_PAIRS and len(a) == len(b) == total, "the oracle's pair list was cut"
    return clusters_of_pairs(vertices, a, b), total


def _same(x, y):
    """Two answers (ids, labels, clusters, members): the same bytes."""
    return x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes() and x[2:] == y[2:]


def _check(st, sa, sb, ids_a, ids_b, bound, other, live=None):
    """The scoped call (sb None: inside sa) against the reduced oracle, exactly; live: the store's live ids (None: every id
    the scopes name is live).  -> ((ids, labels, clusters, members), the oracle's pair count)."""
    named = set(int(i) for i in ids_a) | set(int(i) for i in (ids_b if ids_b is not None else ()))
    vertices = sorted(named if live is None else named & set(live))
    (want, wc, wm), total = _oracle(st, sa, sb, vertices, bound, other)
    got = st.similar_clusters_scoped_raw(bound, other, sa, sb)
    ids, labels, clusters, members = got
    assert ids.dtype == np.uint32 and labels.dtype == np.uint32
    assert ids.tolist() == vertices  # ascending, each once, *out_n of them
    expect = [want[i] for i in vertices]
    bad = [k for k in range(len(vertices)) if labels[k] != expect[k]]
    assert not bad, [(vertices[k], int(labels[k]), expect[k]) for k in bad[:8]]
    assert (clusters, members) == (wc, wm)
    assert st.similar_clusters_info(scoped=True)["vertices"] == len(vertices)
    return got, total


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


@pytest.mark.parametrize("n,dim", [(2, 384), (129, 384), (300, 384), (1000, 384), (300, 768), (300, 1024)])
def test_random_graphs_against_the_oracle(VS, n, dim):
    st = _store(VS, _random_rows(n, dim), groups=_files_of_8(n))
    rng = np.random.default_rng(n + dim)
    planted = [r for r in (0, 9, 10, 127, 128, 140, n - 1) if n >= 200]
    everything = list(range(n))
    half = sorted(set(rng.choice(n, n // 2, replace=False).tolist()) | set(planted))  # packed position != stored row
    rest = sorted(set(everything) - set(half) | ({128} if n >= 200 else set()))        # (128 in both when planted)
    run129 = list(range(5, min(n, 5 + 129)))     # off a tile edge: a ragged last packed tile, on and off the diagonal
    run257 = list(range(37, min(n, 37 + 257)))   # overlaps run129 in 37 .. 133, which holds the planted 127 ~ 128
    lists = {"every": everything, "half": half, "rest": rest, "run129": run129, "run257": run257,
             "co_half": sorted(set(everything) - set(half))}
    sc = {k: st.scope(v) for k, v in lists.items()}
    twin = st.scope(half)  # a second handle of the same ids
    every2 = st.scope(everything)
    for bound in (np.float32(0.12), BOUND):
        for other in (False, True):
            dense = st.similar_clusters_raw(bound, other_files=other)
            # one handle; the all-ids scope passed twice is the unscoped call, in bytes
            for k in ("every", "half", "run129", "run257"):
                got, total = _check(st, sc[k], None, lists[k], None, bound, other)
                print(f"n={n} dim={dim} bound={bound} other={other} {k}: {total} pairs, {got[2]} classes, {got[3]} members")
                if k == "every":
                    assert got[0].tolist() == everything and got[1].tobytes() == dense[0].tobytes() and got[2:] == dense[1:]
                    via = st.similar_clusters_raw(bound, other_files=other, scope=sc[k])
                    assert via[0].tobytes() == dense[0].tobytes() and via[1:] == dense[1:]
                    assert _same(got, st.similar_clusters_scoped_raw(bound, other, sc[k], sc[k]))  # the same handle named twice
                    assert _same(got, st.similar_clusters_scoped_raw(bound, other, sc[k], every2))  # the rectangle of two equal lists
            # two disjoint scopes; two overlapping ones (128 in both; the runs' overlap holds a planted pair); each swapped
            for ka, kb in (("half", "co_half"), ("half", "rest"), ("run129", "run257"), ("run129", "every")):
                got, total = _check(st, sc[ka], sc[kb], lists[ka], lists[kb], bound, other)
                swapped, _ = _check(st, sc[kb], sc[ka], lists[kb], lists[ka], bound, other)
                assert _same(got, swapped), (ka, kb)
            # two different handles holding the same ids give one handle's bytes
            one = st.similar_clusters_scoped_raw(bound, other, sc["half"])
            assert _same(one, st.similar_clusters_scoped_raw(bound, other, sc["half"], twin))
            assert _same(one, st.similar_clusters_scoped_raw(bound, other, twin, sc["half"]))
    if n >= 200:
        ids, labels, clusters, members = st.similar_clusters_scoped_raw(BOUND, False, sc["half"])
        lab = dict(zip(ids.tolist(), labels.tolist()))
        assert lab[n - 1] == 0 and lab[10] == 9 and lab[128] == 127 and lab[140] == 127 and (clusters, members) == (3, 7)
        # run129 x run257: 127 ~ 128 lies in the overlap, 128 ~ 140 has 128 in A and 140 in B; 9 ~ 10 lies in A only
        ids, labels, clusters, members = st.similar_clusters_scoped_raw(BOUND, False, sc["run129"], sc["run257"])
        lab = dict(zip(ids.tolist(), labels.tolist()))
        assert lab[128] == 127 and lab[140] == 127 and lab[10] == 10 and (clusters, members) == (1, 3)
    # no bound at all: a scope is one class; above every cosine: everybody alone
    ids, labels, clusters, members = st.similar_clusters_scoped_raw(None, False, sc["half"])
    assert ids.tolist() == half and (labels == half[0]).all() and (clusters, members) == ((1, len(half)) if len(half) > 1 else (0, 0))
    ids, labels, clusters, members = st.similar_clusters_scoped_raw(2.0, False, sc["half"], sc["every"])
    assert ids.tolist() == everything and labels.tolist() == everything and (clusters, members) == (0, 0)
    st.close()


def test_empty_joins_launch_nothing(VS):
    """A side without a live row, one scope with fewer than two live rows, two handles holding the same single row: every
    vertex its own label, the counts 0, no launch of the join."""
    st = _store(VS, synth_rows(8201, 0, 40, 384), id_base=50)
    none, never, one, same_one, few = st.scope([]), st.scope([500, 501]), st.scope([57]), st.scope([57]), st.scope([60, 61, 62])
    for sa, sb, vertices in ((none, None, []), (none, none, []), (never, few, [60, 61, 62]), (few, none, [60, 61, 62]),
                             (one, None, [57]), (one, same_one, [57]), (same_one, one, [57]), (never, never, [])):
        ids, labels, clusters, members = st.similar_clusters_scoped_raw(-1.0, False, sa, sb)
        assert ids.tolist() == vertices and labels.tolist() == vertices and (clusters, members) == (0, 0)
        info = st.similar_clusters_info(scoped=True)
        assert info["launches"] == 0 and info["tile_pairs_scored"] == 0 and info["vertices"] == len(vertices)
    # two handles, one row each, DIFFERENT rows: a join of one tile pair
    other_one = st.scope([58])
    ids, labels, clusters, members = st.similar_clusters_scoped_raw(-1.0, False, one, other_one)
    assert ids.tolist() == [57, 58] and labels.tolist() == [57, 57] and (clusters, members) == (1, 2)
    info = st.similar_clusters_info(scoped=True)
    assert info["launches"] == 1 and (info["rows_a"], info["rows_b"]) == (1, 1)
    # the info of either kind: an unscoped call zeroes the scoped fields
    st.similar_clusters_raw(0.9)
    info = st.similar_clusters_info(scoped=True)
    assert (info["pack_ms"], info["rows_a"], info["rows_b"], info["vertices"]) == (0.0, 0, 0, 0) and info["launches"] >= 1
    st.similar_clusters_scoped_raw(0.9, False, few, never)
    assert st.similar_clusters_info() == {"tile_pairs_scored": 0, "tile_pairs_skipped": 0, "rescored_pairs": 0, "launches": 0,
                                          "join_ms": 0.0, "label_ms": st.similar_clusters_info()["label_ms"]}
    st.close()


def test_not_the_unscoped_answer_restricted(VS):
    """a ~ x and x ~ b at 0.95, a ~ b about 0.90, the bound 0.93: the unscoped call puts a and b in one class through x; a
    scope of a and b without x leaves each alone — a path through a chunk outside connects nothing — and with x in `other`
    the rectangle joins all three."""
    n, a, b, x = 300, 20, 150, 200
    rows = synth_rows(8400, 0, n, 384).copy()
    _plant(rows, x, a, 0.95)
    _plant(rows, x, b, 0.95)
    st = _store(VS, rows)
    bound = np.float32(0.93)
    cos_ab = float(rows[a].astype(np.float64) @ rows[b].astype(np.float64) /
                   (np.linalg.norm(rows[a].astype(np.float64)) * np.linalg.norm(rows[b].astype(np.float64))))
    assert cos_ab < float(bound) - 2 * MARGIN, cos_ab
    dense = st.similar_clusters_raw(bound)
    assert dense[0][a] == dense[0][b] == dense[0][x] == a and dense[1:] == (1, 3)
    inside = list(range(0, 180))
    sc, sx = st.scope(inside), st.scope([x])
    (ids, labels, clusters, members), total = _check(st, sc, None, inside, None, bound, False)
    assert total == 0 and labels.tolist() == inside and (clusters, members) == (0, 0)
    restricted = dense[0][inside]
    assert restricted[a] == restricted[b]  # what filtering the unscoped labels on the host would have said
    (ids, labels, clusters, members), total = _check(st, sc, sx, inside, [x], bound, False)
    lab = dict(zip(ids.tolist(), labels.tolist()))
    assert total == 2 and lab[a] == lab[b] == lab[x] == a and (clusters, members) == (1, 3)
    assert st.similar_clusters_raw(bound, scope=sc, other=sx)[0][x] == a
    assert st.similar_clusters_raw(bound, scope=sc)[0][x] == NO_ID  # outside A u B
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


HOG_SCOPE = list(range(100)) + list(range(200, 800)) + [900]  # 100 other rows, the file, its copy


@pytest.fixture(scope="module")
def hog_store(VS):
    rows, hog, groups = _hog_rows()
    st = _store(VS, rows, groups=groups)
    yield st
    st.close()


def test_a_hog_inside_the_scope_is_one_class_not_a_refusal(hog_store):
    st = hog_store
    hog = np.arange(200, 800)
    sc = st.scope(HOG_SCOPE)
    with pytest.raises(_lib.CsError, match="candidate pairs") as e:
        st.similar_pairs_raw(BOUND, other_files=False, max_pairs=2000, scope=sc)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    first = st.similar_clusters_scoped_raw(BOUND, False, sc)
    ids, labels, clusters, members = first
    assert ids.tolist() == HOG_SCOPE and (clusters, members) == (1, 601)  # known by construction
    lab = dict(zip(ids.tolist(), labels.tolist()))
    assert all(lab[int(r)] == 200 for r in hog) and lab[900] == 200 and all(lab[r] == r for r in range(100))
    _check(st, sc, None, HOG_SCOPE, None, BOUND, False)  # the oracle with room: 180,300 pairs
    for _ in range(2):  # three calls: identical bytes, however the unions raced
        assert _same(first, st.similar_clusters_scoped_raw(BOUND, False, sc))
    # OTHER_GROUP: no edge inside the file, and still one class through the copy in the other file
    (ids, labels, clusters, members), total = _check(st, sc, None, HOG_SCOPE, None, BOUND, True)
    assert total == 600 and (clusters, members) == (1, 601)
    # the same hog OUTSIDE the scope changes nothing for a scope of the rest
    rest = sorted(set(range(1000)) - set(hog.tolist()) - {900})
    sr = st.scope(rest)
    (ids, labels, clusters, members), total = _check(st, sr, None, rest, None, BOUND, False)
    assert total == 0 and labels.tolist() == rest and (clusters, members) == (0, 0)
    # the file against the rest: only the copy crosses
    sh = st.scope(hog.tolist())
    both = sorted(rest + [900])
    s9 = st.scope(both)
    (ids, labels, clusters, members), total = _check(st, sh, s9, hog.tolist(), both, BOUND, False)
    assert total == 600 and (clusters, members) == (1, 601)


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


# the planted set cut in two so that every planted pair crosses: the pairs' second ids, the spokes and two of the twins in B
SIDE_B = sorted({b for _, b in SPOTS} | set(SPOKES) | set(TWINS[1:]) |
                {r for r in range(1, 1000, 2) if r not in {a for a, _ in SPOTS} | {HUB, TWINS[0]}})
SIDE_A = sorted(set(range(1000)) - set(SIDE_B))


@pytest.fixture(scope="module")
def planted_store(VS):
    st = _store(VS, _planted(), groups=_files_of_8(1000))
    yield st
    st.close()


def test_planted_pairs_around_the_bound(planted_store):
    """Planted pairs at the bound +- margin / 2 (the rescore decides them) and +- 2 margin (above: united without a rescore;
    below: ruled out by the f16 product), in the triangle of one scope and in the rectangle of two."""
    st = planted_store
    every, sa, sb = st.scope(range(1000)), st.scope(SIDE_A), st.scope(SIDE_B)
    for s1, s2, l1, l2 in ((every, None, list(range(1000)), None), (sa, sb, SIDE_A, SIDE_B)):
        (ids, labels, clusters, members), total = _check(st, s1, s2, l1, l2, BOUND, False)
        lab = dict(zip(ids.tolist(), labels.tolist()))
        for (a, b), d in zip(SPOTS, DELTAS):
            assert (lab[b] == a) == (d > 0), (a, b, d)
            assert lab[a] == a
        assert all(lab[s] == HUB for s in SPOKES)
        assert st.similar_clusters_info()["rescored_pairs"] >= 4  # the four at +- margin / 2 at least
        _check(st, s1, s2, l1, l2, BOUND, True)
        _check(st, s1, s2, l1, l2, np.float32(0.15), False)
    # in the triangle the twins and the spokes' mutual pairs count too; in the rectangle the twins 971 ~ 972 do not cross
    assert st.similar_clusters_scoped_raw(BOUND, False, every)[2:] == (4 + 1 + 1, 8 + 12 + 3)


def test_the_bound_is_strict_at_equal_bits(planted_store):
    st = planted_store
    pa, pb = SPOTS[0]  # planted at the bound + margin / 2
    every, sa, sb = st.scope(range(1000)), st.scope(SIDE_A), st.scope(SIDE_B)
    cos, a, b, total = st.similar_pairs_raw(np.float32(0.85), max_pairs=ORACLE_PAIRS, scope=every)
    exact = np.float32(cos[[i for i in range(total) if (a[i], b[i]) == (pa, pb)][0]])  # the pair's f32 cosine
    assert abs(float(exact) - (0.9 + MARGIN / 2)) < 1e-6
    for s1, s2, l1, l2 in ((every, None, list(range(1000)), None), (sa, sb, SIDE_A, SIDE_B)):
        def label_of_pb(bound):
            ids, labels, _c, _m = st.similar_clusters_scoped_raw(bound, False, s1, s2)
            return int(labels[ids.tolist().index(pb)])
        assert label_of_pb(exact) == pb  # equal bits: no edge
        assert label_of_pb(np.nextafter(exact, np.float32(-1))) == pa  # one ulp under the cosine
        assert label_of_pb(np.nextafter(exact, np.float32(2))) == pb
        for bound in (exact, np.nextafter(exact, np.float32(-1))):
            _check(st, s1, s2, l1, l2, bound, False)


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


EQUI = list(range(150, 530))  # where the 380 equi-cosine rows sit in a store of 700


def _equi_store_rows():
    rows = synth_rows(8500, 0, 700, 384).copy()
    rows[150:530] = _equi_cosine()
    return rows


def _equi_cases(st):
    """-> [(scope_a, scope_b, ids_a, ids_b, the set's pairs the join holds, its tile pairs)]: the set as one scope (the
    triangle of 3 packed tiles), and split odd / even into two (the rectangle of 2 x 2)."""
    odd, even = EQUI[1::2], EQUI[0::2]
    return [(st.scope(EQUI), None, EQUI, None, 380 * 379 // 2, 6), (st.scope(odd), st.scope(even), odd, even, 190 * 190, 4)]


def test_an_equi_cosine_set_is_all_ambiguous(VS):
    """380 rows at stored rows 150 .. 529 of a larger store, every pair at the bound itself: none can be decided by the f16
    product, all go through the buffer and the rescore, and f32 rounding puts some on each side."""
    st = _store(VS, _equi_store_rows())
    for sa, sb, la, lb, set_pairs, tile_pairs in _equi_cases(st):
        got, total = _check(st, sa, sb, la, lb, BOUND, False)
        print(f"equi-cosine {'triangle' if sb is None else 'rectangle'}: {total} of {set_pairs} pairs above the bound, "
              f"{got[2]} classes, {got[3]} members")
        assert 0 < total < set_pairs, "the set no longer straddles the bound: the test's data needs another look"
        info = st.similar_clusters_info(scoped=True)
        assert info["rescored_pairs"] > 0 and info["tile_pairs_scored"] + info["tile_pairs_skipped"] == tile_pairs
        assert info["launches"] == 2  # the first tile row, then the rest
        for _ in range(2):  # three calls: identical bytes
            assert _same(got, st.similar_clusters_scoped_raw(BOUND, False, sa, sb))
    st.close()


def test_many_launches_and_an_overflowing_buffer_change_nothing(lab_lib, VS, monkeypatch):
    """Two laboratory knobs (the diagnostic library reads them) reach the paths a small scope never takes by itself: a
    launch of two tile pairs, and the ambiguous buffer at its minimum of one tile pair's worth — the equi-cosine set's
    first launch then holds more than 16,384 ambiguous pairs, in the triangle and in the rectangle, and is split."""
    rows, hog, groups = _hog_rows()
    equi, hogs = _store(VS, _equi_store_rows()), _store(VS, rows, groups=groups)
    cases = _equi_cases(equi) + [(hogs.scope(HOG_SCOPE), None, HOG_SCOPE, None, None, 21)]  # 701 rows: 6 packed tiles
    stores = [equi, equi, hogs]
    default = [[st.similar_clusters_scoped_raw(BOUND, other, c[0], c[1]) for other in (False, True)] for st, c in zip(stores, cases)]
    launches = []
    for st, c in zip(stores, cases):
        st.similar_clusters_scoped_raw(BOUND, False, c[0], c[1])
        launches.append(st.similar_clusters_info()["launches"])
    monkeypatch.setenv("CS_CLUSTERS_LAUNCH_TILE_PAIRS", "2")
    monkeypatch.setenv("CS_CLUSTERS_AMBIGUOUS_CAP", "1")
    for st, c, want, before in zip(stores, cases, default, launches):
        for other in (False, True):
            got = st.similar_clusters_scoped_raw(BOUND, other, c[0], c[1])
            assert _same(got, want[other])
            info = st.similar_clusters_info()
            print(info)
            assert info["tile_pairs_scored"] + info["tile_pairs_skipped"] == c[5]
            if not other:
                assert info["launches"] > before
    # the equi-cosine set: the launch (0,0)+(0,1) overflowed and was repeated as halves: more launches than tile pairs / 2
    for c in cases[:2]:
        equi.similar_clusters_scoped_raw(BOUND, False, c[0], c[1])
        assert equi.similar_clusters_info()["launches"] > c[5] // 2
    # the hog: packed tiles 1..4 hold nothing but the file, and are one class after their first tile row
    hogs.similar_clusters_scoped_raw(BOUND, False, cases[2][0])
    assert hogs.similar_clusters_info()["tile_pairs_skipped"] > 0
    equi.close()
    hogs.close()


def test_id_base_deleted_rows_and_the_refresh(VS, monkeypatch):
    """id_base = 1,000; the scopes are made before 30 % of the rows are deleted — a class's smallest member and ids the
    scopes name among them; both states a built index can be in (tombstones kept: CS_INDEX_COMPACT_DEAD_PCT=0; reclaimed:
    the rows move, the ids stay) give the same bytes.  The call refreshes the lists, once."""
    n, base = 1000, 1000
    rows = _planted()
    groups = _files_of_8(n, base)
    rng = np.random.default_rng(11)
    protect = set(SPOKES + TWINS[1:] + [x for p in SPOTS for x in p])
    pool = [r for r in range(n) if r not in protect and r not in (HUB, TWINS[0])]
    gone_rows = sorted(set(rng.choice(pool, (3 * n) // 10 - 2, replace=False).tolist()) | {HUB, TWINS[0]})
    gone = [base + r for r in gone_rows]
    live = [base + r for r in range(n) if r not in set(gone_rows)]
    all_ids = [base + r for r in range(n)]
    third = sorted({base + r for r in range(0, n, 3)} | {base + r for r in protect} | {base + HUB, base + TWINS[0]})
    upper = [base + r for r in range(500, n)] + [base + n + 5, base + n + 9]  # and two ids never issued
    answers = []
    for reclaim in (False, True):
        if not reclaim:
            monkeypatch.setenv("CS_INDEX_COMPACT_DEAD_PCT", "0")
        else:
            monkeypatch.delenv("CS_INDEX_COMPACT_DEAD_PCT")
        st = _store(VS, rows, id_base=base, groups=groups)
        every, s3, sup, doomed = st.scope(all_ids), st.scope(third), st.scope(upper), st.scope(gone[:20])
        (ids, labels, clusters, members), _ = _check(st, every, None, all_ids, None, BOUND, False)  # id_base alone
        lab = dict(zip(ids.tolist(), labels.tolist()))
        assert all(lab[base + s] == base + HUB for s in SPOKES) and labels.min() >= base
        _check(st, s3, sup, third, upper, BOUND, False, live=all_ids)
        made = [s.info()[2] for s in (every, s3, sup, doomed)]
        assert made == [1, 1, 1, 1]
        assert st.delete_chunks(gone) == len(gone)
        with pytest.raises(_lib.CsError, match="Index not built"):
            st.similar_clusters_scoped_raw(BOUND, False, every)
        st.build_index()
        assert st.stored_rows() == (n - len(gone) if reclaim else n) and len(st) == n - len(gone)
        assert [s.info()[2] for s in (every, s3, sup, doomed)] == made  # nothing refreshed yet
        got, _ = _check(st, every, None, all_ids, None, BOUND, False, live=live)
        assert every.info() == (n, n - len(gone), 2)  # the call remade the list, once
        ids, labels, clusters, members = got
        assert ids.tolist() == live  # deleted ids are no vertices
        lab = dict(zip(ids.tolist(), labels.tolist()))
        # the hub is gone: the spokes are still clones of each other (0.97^2), labelled by the smallest of them
        assert all(lab[base + s] == base + SPOKES[0] for s in SPOKES)
        assert lab[base + TWINS[1]] == lab[base + TWINS[2]] == base + TWINS[1]
        dense = st.similar_clusters_raw(BOUND)
        assert st.similar_clusters_raw(BOUND, scope=every)[0].tobytes() == dense[0].tobytes() and got[2:] == dense[1:]
        between, _ = _check(st, s3, sup, third, upper, BOUND, False, live=live)
        assert s3.info()[2] == 2 and sup.info()[2] == 2
        inside, _ = _check(st, s3, None, third, None, BOUND, True, live=live)
        low, _ = _check(st, s3, every, third, all_ids, np.float32(0.15), False, live=live)
        assert every.info()[2] == 2
        # only deleted ids: no vertex, no launch — and the list was still refreshed
        assert st.similar_clusters_scoped_raw(None, False, doomed)[0].size == 0 and doomed.info() == (20, 0, 2)
        ids, labels, clusters, members = st.similar_clusters_scoped_raw(None, False, doomed, s3)
        assert ids.tolist() == [i for i in third if i in set(live)] and (labels == ids).all() and (clusters, members) == (0, 0)
        assert st.similar_clusters_info()["launches"] == 0
        answers.append([x.tobytes() for r in (got, between, inside, low) for x in r[:2]] + [r[2:] for r in (got, between, inside, low)])
        st.close()
    assert answers[0] == answers[1]  # tombstoned or reclaimed: the same labels


def test_scoped_clusters_beside_searches(hog_store):
    """At most four threads through the same two scopes beside ordinary searches: every answer equals the serial one."""
    st = hog_store
    hog = list(range(200, 800))
    sc, sh, s9 = st.scope(HOG_SCOPE), st.scope(hog), st.scope(list(range(100)) + [900])
    qs = synth_rows(7701, 0, 3, 384)
    want_in, want_x, want_search = (st.similar_clusters_scoped_raw(BOUND, False, sc), st.similar_clusters_scoped_raw(BOUND, False, sh, s9),
                                    st.search_raw(qs, 10))
    assert want_x[2:] == (1, 601)
    errors = []

    def clusters(swap):
        try:
            for _ in range(6):
                if not _same(st.similar_clusters_scoped_raw(BOUND, False, sc), want_in):
                    errors.append("inside")
                if not _same(st.similar_clusters_scoped_raw(BOUND, False, *((s9, sh) if swap else (sh, s9))), want_x):
                    errors.append("between")
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

    th = [threading.Thread(target=clusters, args=(False,)), threading.Thread(target=search),
          threading.Thread(target=clusters, args=(True,)), threading.Thread(target=clusters, args=(False,))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors


class _Out:
    """Output buffers prefilled with a pattern: a failing call writes nothing."""

    def __init__(self, room):
        self.ids = np.full(room, 0xA5A5A5A5, np.uint32)
        self.labels = np.full(room, 0x5A5A5A5A, np.uint32)
        self.n = ctypes.c_uint64(0x6666)
        self.clusters = ctypes.c_uint64(0x7777)
        self.members = ctypes.c_uint64(0x8888)

    def untouched(self):
        return ((self.ids == 0xA5A5A5A5).all() and (self.labels == 0x5A5A5A5A).all() and self.n.value == 0x6666
                and self.clusters.value == 0x7777 and self.members.value == 0x8888)


def _raw(lib, h, sa, sb, min_cos, mode, o, cap, ids=True, labels=True, n=True):
    return lib.cs_index_similar_clusters_scoped(h, sa, sb, min_cos, mode, o.ids.ctypes.data_as(_lib.u32p) if ids else None,
                                                o.labels.ctypes.data_as(_lib.u32p) if labels else None, cap,
                                                ctypes.byref(o.n) if n else None, ctypes.byref(o.clusters), ctypes.byref(o.members))


def test_errors_and_their_order(VS, gpu_lib, monkeypatch):
    n, dim = 500, 384
    st = VS(None, dim)
    st.insert_embeddings(synth_rows(7601, 0, n, dim))
    elsewhere = _store(VS, synth_rows(7605, 0, 64, dim))
    sc, small, foreign = st.scope(range(0, n, 2)), st.scope([3, 4, 5]), elsewhere.scope(range(64))
    o = _Out(n)
    nan = float("nan")
    H = lambda s: s.handle if s is not None else None

    def fails(code, text, sa, sb, *args, handle=True, **kw):
        before = [s.info()[2] for s in (sc, small, foreign)]
        assert _raw(gpu_lib, st.handle if handle else None, H(sa), H(sb), *args, **kw) == code
        assert text in _lib.last_error(), _lib.last_error()
        assert o.untouched()                                              # a failing call writes nothing
        assert [s.info()[2] for s in (sc, small, foreign)] == before      # and refreshes no list

    bad = _lib.CS_ERR_BAD_ARG
    # 1. the handle and the built state, with the unscoped clusters call's texts, before everything behind them
    fails(bad, "null index handle", None, None, nan, 9, o, 0, handle=False, ids=False)
    fails(_lib.CS_ERR_NOT_BUILT, "Index not built. Call build_index() after inserting chunks.", None, None, nan, 9, o, 0, ids=False)
    st.build_index()
    # 2. a null out_ids, out_label or out_n, before the mode
    fails(bad, "null buffer", None, None, nan, 9, o, 0, ids=False)
    fails(bad, "null buffer", sc, foreign, nan, 9, o, 0, labels=False)
    fails(bad, "null buffer", None, sc, nan, 9, o, 0, n=False)
    # 3. the mode, before the bound;  4. the bound, before the scopes
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", None, None, nan, 2, o, 0)
    fails(bad, "mode must be CS_PAIRS_ALL or CS_PAIRS_OTHER_GROUP", sc, sc, nan, -1, o, 0)
    fails(bad, "min_cos is NaN", None, foreign, nan, 1, o, 0)
    # 5. a null scope_a, then a null scope_b: the text says which.  NULL does not mean "the whole store"
    fails(bad, "null scope handle (scope_a)", None, None, 0.5, 0, o, 0)
    fails(bad, "null scope handle (scope_a)", None, foreign, 0.5, 0, o, 0)
    fails(bad, "null scope handle (scope_b)", sc, None, 0.5, 0, o, 0)
    fails(bad, "null scope handle (scope_b)", foreign, None, 0.5, 0, o, 0)
    # 6. a scope made for another store, on either side, before cap
    fails(bad, "the scope was made for another store", foreign, sc, 0.5, 0, o, 0)
    fails(bad, "the scope was made for another store", sc, foreign, 0.5, 0, o, 0)
    fails(bad, "the scope was made for another store", foreign, foreign, 0.5, 0, o, 0)
    # 7. cap: n_ids(scope_a) + (same handle ? 0 : n_ids(scope_b)), off by one; the text names the number wanted
    fails(bad, f"= {n // 2} ", sc, sc, 0.5, 0, o, n // 2 - 1)
    fails(bad, f"= {n // 2 + 3} ", sc, small, 0.5, 0, o, n // 2 + 2)
    fails(bad, f"= {n // 2 + 3} ", small, sc, 0.5, 1, o, n // 2 + 2)
    fails(bad, "= 3 ", small, small, 0.5, 0, o, 2)
    assert "cap must be at least" in _lib.last_error() and "got 2" in _lib.last_error()
    assert sc.info()[2] == 0  # the list is still to be made: no failing call made it
    assert _raw(gpu_lib, st.handle, sc.handle, small.handle, 0.5, 1, o, n // 2 + 3) == _lib.CS_OK
    assert (o.n.value, o.clusters.value, o.members.value) == (n // 2 + 2, 0, 0)  # 4 is in both
    assert sc.info()[2] == 1 and small.info()[2] == 1 and sc.route_info()[:3] == (0, 0, 0) and small.route_info()[:3] == (0, 0, 0)
    want = sorted(set(range(0, n, 2)) | {3, 5})
    assert o.ids[:len(want)].tolist() == want and o.labels[:len(want)].tolist() == want
    assert (o.ids[len(want):] == 0xA5A5A5A5).all() and (o.labels[len(want):] == 0x5A5A5A5A).all()  # nothing past *out_n
    # the counts are optional
    assert gpu_lib.cs_index_similar_clusters_scoped(st.handle, small.handle, small.handle, 0.5, 0, o.ids.ctypes.data_as(_lib.u32p),
                                                    o.labels.ctypes.data_as(_lib.u32p), 3, ctypes.byref(o.n), None, None) == _lib.CS_OK
    assert o.n.value == 3
    # 8. a dim the f16 filter has no tiles for — behind the scopes and behind cap
    odd = VS(None, 100)
    odd.insert_embeddings(synth_rows(7602, 0, 50, 100))
    odd.build_index()
    so = odd.scope(range(50))
    made = so.info()[2]  # (a scope made over a built index has its list already)
    o = _Out(64)
    call = lambda sa, sb, cap: _raw(gpu_lib, odd.handle, H(sa), H(sb), 0.5, 0, o, cap)
    assert call(so, None, 50) == bad and "null scope handle (scope_b)" in _lib.last_error()
    assert call(so, sc, 50) == bad and "the scope was made for another store" in _lib.last_error()
    assert call(so, so, 49) == bad and "cap must be at least" in _lib.last_error() and o.untouched()
    assert call(so, so, 50) == _lib.CS_ERR_UNSUPPORTED
    assert "similar clusters need dim 384, 768 or 1024" in _lib.last_error() and "got 100" in _lib.last_error() and o.untouched()
    assert so.info()[2] == made
    odd.close()
    # ... then CS_INDEX_SPLIT=0, which turned the filter copies off: refused like the unscoped call, before the list is made
    monkeypatch.setenv("CS_INDEX_SPLIT", "0")
    off = VS(None, dim)
    off.insert_embeddings(synth_rows(7603, 0, 50, dim))
    off.build_index()
    sf = off.scope(range(50))
    made = sf.info()[2]
    assert _raw(gpu_lib, off.handle, sf.handle, sf.handle, 0.5, 0, o, 50) == _lib.CS_ERR_UNSUPPORTED
    assert "similar clusters need the f16 filter copy, and CS_INDEX_SPLIT=0" in _lib.last_error() and o.untouched()
    assert sf.info()[2] == made
    off.close()
    monkeypatch.delenv("CS_INDEX_SPLIT")
    # the Python layer
    with pytest.raises(ValueError, match="other= needs scope="):
        st.similar_clusters_raw(0.9, other=sc)
    with pytest.raises(_lib.CsError, match="the scope was made for another store"):
        st.similar_clusters_raw(0.9, scope=sc, other=foreign)
    done = st.scope([1, 2])
    done.close()
    with pytest.raises(_lib.CsError, match="scope is closed"):
        st.similar_clusters_raw(0.9, scope=done)
    st.close()
    elsewhere.close()


def test_a_sharded_store_and_its_scopes_are_refused(VS):
    dim = 384
    st = _store(VS, synth_rows(9933, 0, 64, dim))
    sharded = VS(None, dim, devices=[0, 0])
    sharded.insert_embeddings(synth_rows(9934, 0, 64, dim))
    sharded.build_index()
    over_shards = sharded.scope(np.arange(64))
    with pytest.raises(_lib.CsError, match="no similar-clusters search: no cs_shards_ form yet") as e:
        sharded.similar_clusters_raw(0.9, scope=over_shards)
    assert e.value.code == _lib.CS_ERR_UNSUPPORTED
    mine = st.scope(np.arange(64))
    for kw in (dict(scope=over_shards), dict(scope=mine, other=over_shards), dict(scope=over_shards, other=mine)):
        with pytest.raises(_lib.CsError, match="the scope was made for another store") as e:
            st.similar_clusters_raw(0.9, **kw)
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
    for sa, sb, rows in ((sc, sc, n), (half, sc, n // 2)):
        o = _Out(n + n // 2)
        assert _raw(st._lib, st.handle, sa.handle, sb.handle, 0.9, 0, o, n + n // 2) == _lib.CS_ERR_OOM
        bytes_wanted = ((rows + 127) // 128) * 128 * 384 * 2  # the first side's packed tiles
        assert f"no room for the f16 filter copy ({bytes_wanted} bytes)" in _lib.last_error(), _lib.last_error()
        assert o.untouched()
    monkeypatch.delenv("CS_FAULT_F16_ALLOC")
    ids, labels, clusters, members = st.similar_clusters_scoped_raw(0.9, False, half, sc)  # the handle and the scopes live on
    assert ids.tolist() == list(range(n)) and (clusters, members) == (0, 0)
    st.close()


def test_no_trace_where_the_int8_copy_serves(VS):
    """5,000 rows: the int8 copy serves the index, which holds no f16 copy — the call packs its own buffers and leaves the
    index and the scopes as they were: the same filter state and copies, the same bits from a search on the default route,
    the scopes' route counters where they stood."""
    n, dim = 5000, 384
    rows = synth_rows(7501, 0, n, dim).copy()
    spots = [(5, 4999), (127, 128), (3000, 3001), (4990, 4995), (2047, 2048), (128, 4000)]
    for i, (a, b) in enumerate(spots):
        _plant(rows, a, b, 0.9 + [2e-4, -2e-4, 5e-4, -5e-4, 0.05, 0.03][i])
    st = _store(VS, rows, groups=_files_of_8(n))
    assert st.filter_state()[0] == 2 and st.filter_copies()[:2] == (True, False)
    odd = sorted(set(range(1, n, 2)) | {r for p in spots for r in p})
    tail = list(range(2000, n))
    s_odd, s_tail = st.scope(odd), st.scope(tail)
    qs = synth_rows(7502, 0, 6, dim)
    state, copies, before = st.filter_state(), st.filter_copies(), st.search_raw(qs, 10)
    routes = (s_odd.route_info(), s_tail.route_info())
    first = st.similar_clusters_scoped_raw(BOUND, False, s_odd)
    lab = dict(zip(first[0].tolist(), first[1].tolist()))
    assert first[2:] == (4, 8) and lab[4999] == 5 and lab[3001] == 3000 and lab[2048] == 2047 and lab[4000] == 128
    assert lab[128] == 128 and lab[4995] == 4995  # 127 ~ 128 and 4990 ~ 4995 were planted under the bound
    cross = st.similar_clusters_scoped_raw(BOUND, False, s_odd, s_tail)
    for _ in range(2):  # the same calls three times: identical bytes
        assert _same(first, st.similar_clusters_scoped_raw(BOUND, False, s_odd))
        assert _same(cross, st.similar_clusters_scoped_raw(BOUND, False, s_tail, s_odd))
    assert st.filter_state() == state and st.filter_copies() == copies
    assert (s_odd.route_info(), s_tail.route_info()) == routes
    after = st.search_raw(qs, 10)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(before, after))
    for other in (False, True):  # few pairs: the oracle call is neither refused nor cut (asserted)
        _check(st, s_odd, None, odd, None, BOUND, other)
        _check(st, s_odd, s_tail, odd, tail, BOUND, other)
    assert st.filter_state() == state and st.filter_copies() == copies and (s_odd.route_info(), s_tail.route_info()) == routes
    st.close()


def _file_chunks(rows, paths):
    from codesearch_amd import Chunk, EmbeddedChunk

    return [EmbeddedChunk(Chunk(f"chunk {i}", i, i + 1, "Function", p), rows[i]) for i, p in enumerate(paths)]


def test_similar_clusters_in_a_directory_with_metadata(VS):
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
    src, vendor = st.scope(st.chunk_ids_under("src/")), st.scope(st.chunk_ids_under("vendor/"))
    assert [[r.id for r in c] for c in st.similar_clusters(0.95)] == [[1, 6, 13], [3, 10]]
    # under src/ alone: 1 and 13 are clones of each other (0.99^2) but one file; 4 ~ 8 is one file too
    assert st.similar_clusters(0.95, scope=src) == []
    inside = st.similar_clusters(0.95, other_files=False, scope=src)
    assert [[r.id for r in c] for c in inside] == [[1, 13], [4, 8]]
    assert [r.path for r in inside[0]] == ["src/b.rs", "src/b.rs"] and inside[1][1].content == "chunk 8"
    # src/ against vendor/: the class of three; 3 ~ 10 has its other end under lib/
    across = st.similar_clusters(0.95, scope=src, other=vendor)
    assert [[r.id for r in c] for c in across] == [[1, 6, 13]]
    assert [r.path for r in across[0]] == ["src/b.rs", "vendor/copy.rs", "src/b.rs"]
    assert [[r.id for r in c] for c in st.similar_clusters(0.95, scope=vendor, other=src)] == [[1, 6, 13]]
    assert len(st.similar_clusters(0.95, scope=src, other=vendor, min_size=1)) == 1 + (20 - 2) + (10 - 1)
    st.close()


def test_cpp_wrapper_reports_scoped_clone_classes():
    """host/codesearch_gpu.hpp: the scoped VectorStore::similar_clusters (tests/cpp/similar_clusters_scoped_host_test.cpp)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tests", "cpp", "similar_clusters_scoped_host_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "similar_clusters_scoped_host_test")
    lib_dir = os.path.join(root, "codesearch_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", src, "-o", exe, f"-L{lib_dir}", "-lcsgpu",
                    f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "similar clusters scoped host ok" in r.stdout
