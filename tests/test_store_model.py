"""Pins tests/store_model.py on the CPU: the model's bookkeeping, its judge against the C oracle's answers — and against
hand-made WRONG answers, each of which it must reject: a judge that accepts everything is the failure this file guards
against — and the coverage of every walk the GPU test runs (tests/test_gpu_store_walk.py).  Below, the same for the kinds
that start from stored rows and for the boosted search: the judges check_similar, check_pairs, check_clusters and
check_boosted, and the extended walks of tests/test_gpu_store_walk_similar.py."""
import json
import os

import numpy as np
import pytest

from codesearch_amd.synth import synth_planted, synth_rows
from tests.store_model import (BOUND, CHAIN, EDGES, LADDER, NO_CLASS, NO_GROUP, NO_ID, NOT_BUILT, WALKS, StoreModel,
                               apply, clone_layout, extended_coverage, make_walk, new_model, plant, required_coverage, resolve,
                               rows_of, tolerance, walk_coverage)

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "scan_golden.json")))


def _padded(cos, ids, k):
    c, i = np.zeros(k, np.float32), np.full(k, NO_ID, np.uint32)
    c[:len(cos)], i[:len(ids)] = cos, ids
    return c, i, len(ids)


def test_tolerance_is_the_derived_bound():
    assert tolerance(384) == 2 * 392 * 2.0 ** -24 and 4.6e-5 < tolerance(384) < 4.7e-5
    assert StoreModel(100).tol == 2 * 108 * 2.0 ** -24


def test_golden_cases_pass_the_judge(oracle):
    """The committed golden answers (float64 order) are the model's own top-k, and the oracle's f32 answers pass its
    check.  (The 100,000-row corpus is left to test_oracle_scan.py: the model keeps a float64 copy of what it holds.)"""
    models = {}
    seen = 0
    for case in GOLDEN["cases"]:
        n, dim, seed, k = case["n"], case["dim"], case["seed"], case["k"]
        if n > 5000:
            continue
        if (n, dim, seed) not in models:
            m = StoreModel(dim)
            m.insert(oracle.synth_rows(seed, 0, n, dim))
            m.build()
            models[(n, dim, seed)] = m
        m = models[(n, dim, seed)]
        if case["kind"] == "random":
            q = synth_rows(case["query_seed"], case["qi"], 1, dim)[0]
        else:
            q = synth_planted(seed, case["query_seed"], [case["planted_row"]] * (case["qi"] + 1), dim)[case["qi"]]
        assert m.topk(q, k)[1].tolist() == case["ids"]
        corpus = np.stack([m.rows[i] for i in range(n)])
        for mode in ("literal", "omp"):
            err = m.check(q, k, _padded(*oracle.scan_topk(corpus, q, k, mode=mode), k))
            assert err <= m.tol
        seen += 1
    assert seen == 50


@pytest.fixture(scope="module")
def big(oracle):
    """5,000 x 384 at id_base 1000, every seventh row tombstoned: (model, corpus, dead bitmap)."""
    n, dim = 5000, 384
    corpus = oracle.synth_rows(31, 0, n, dim)
    m = StoreModel(dim, id_base=1000)
    m.insert(corpus)
    m.build()
    gone = list(range(1000, 1000 + n, 7))
    assert m.delete(gone) == len(gone) and m.delete(gone) == 0
    m.build()
    assert m.stored_rows() == len(m) == n - len(gone)  # 14 % dead: reclaimed
    dead = np.zeros((n + 31) // 32, np.uint32)
    for i in gone:
        dead[(i - 1000) >> 5] |= np.uint32(1 << ((i - 1000) & 31))
    return m, corpus, dead


def test_oracle_answers_pass_on_a_synthetic_corpus(oracle, big):
    m, corpus, dead = big
    n, dim = corpus.shape
    qs = np.concatenate([synth_rows(32, 0, 3, dim), synth_planted(31, 33, [1, 4242], dim), np.zeros((1, dim), np.float32)])
    for q in qs:
        for k in (1, 10, 200):
            got = _padded(*oracle.scan_topk(corpus, q, k, dead=dead, id_base=1000, mode="omp"), k)
            assert m.check(q, k, got) <= m.tol
            mine = m.topk(q, k)
            assert m.check(q, k, mine) <= 1e-7  # (its own answer, rounded to f32)
            if q.any():
                assert mine[1].tolist() == oracle.scan_topk(corpus, q, k, dead=dead, id_base=1000, mode="f64")[1].tolist()
    # an allowed set: the oracle scans with everything else tombstoned
    allowed = np.arange(1000 + 100, 1000 + 900)
    mask = dead.copy()
    for r in list(range(100)) + list(range(900, n)):
        mask[r >> 5] |= np.uint32(1 << (r & 31))
    got = _padded(*oracle.scan_topk(corpus, qs[0], 50, dead=mask, id_base=1000, mode="omp"), 50)
    assert m.check(qs[0], 50, got, allowed=allowed) <= m.tol
    with pytest.raises(AssertionError, match="left out"):  # ... and is not the answer over everything
        m.check(qs[0], 50, got)
    # k above what is live: every live row once, an empty tail
    small = StoreModel(dim)
    small.insert(corpus[:40])
    small.build()
    got = _padded(*oracle.scan_topk(corpus[:40], qs[0], 64, mode="omp"), 64)
    assert got[2] == 40 and small.check(qs[0], 64, got) <= small.tol


@pytest.fixture(scope="module")
def little():
    """600 x 384 at id_base 50 in groups of 16, with exact duplicates and a zero row; ids 50..109 deleted and reclaimed,
    id 200 deleted and still a tombstone."""
    dim = 384
    rows = synth_rows(41, 0, 600, dim)
    rows[300], rows[301], rows[450] = rows[120], rows[120], rows[120]   # ids 170 = 350 = 351 = 500
    rows[130] = 0.0
    m = StoreModel(dim, id_base=50)
    ids = m.insert(rows)
    assert ids == list(range(50, 650))
    m.set_groups(ids, [(i - 50) // 16 for i in ids])
    m.build()
    assert m.delete(range(50, 110)) == 60
    assert m.build() and m.stored_rows() == 540
    assert m.delete([200, 60, 49, 650, 5000]) == 1
    assert not m.build() and m.stored_rows() == 540 and len(m) == 539
    q = (rows[120] + 0.3 * rows[20]).astype(np.float32)   # near the duplicates
    return m, rows, q


def _mutations(m, q):
    """(name, k, answer, allowed, per_file, message) — each answer is wrong in one way."""
    k = 10
    cos, ids, cnt = m.topk(q, k)
    assert ids[:4].tolist() == [170, 350, 351, 500] and cnt == k
    c20, i20, _ = m.topk(q, 20)
    out = []

    def add(name, c, i, n=k, kk=k, allowed=None, per_file=None, match=""):
        out.append((name, kk, (np.asarray(c, np.float32), np.asarray(i, np.uint32), n), allowed, per_file, match))

    add("ids shifted by one", cos, ids + 1, match="cos of id|left out|never issued|deleted")
    i = ids.copy(); i[9] = 200
    add("a deleted id", cos, i, match="id 200 is deleted")
    i = ids.copy(); i[9] = 60
    add("a stale id of a reclaimed row", cos, i, match="id 60 was deleted and reclaimed")
    i = ids.copy(); i[9] = 650
    add("an id never issued", cos, i, match="id 650 was never issued")
    i = ids.copy(); i[9] = 49
    add("an id below id_base", cos, i, match="never issued")
    allowed = [int(x) for x in ids[:9]] + list(range(400, 640))
    assert int(ids[9]) not in allowed
    add("an id outside the mask", cos, ids, allowed=allowed, match="outside the allowed set")
    assert m.groups[350] == m.groups[351]
    add("a group over its cap", cos, ids, per_file=1, match="appears more than 1 times")
    add("the true top-1 missing", np.concatenate([cos[1:], c20[10:11]]), np.concatenate([ids[1:], i20[10:11]]), match="left out|lower id")
    c, i = cos.copy(), ids.copy()
    c[[5, 8]], i[[5, 8]] = c[[8, 5]], i[[8, 5]]
    assert abs(float(cos[5] - cos[8])) > 2 * m.tol
    add("a swapped pair, cosines with their ids", c, i, match="not sorted")
    i = ids.copy(); i[[5, 8]] = i[[8, 5]]
    add("a swapped pair, ids alone", cos, i, match="cos of id")
    i = ids.copy(); i[[1, 2]] = i[[2, 1]]
    add("duplicates in descending id order", cos, i, match="not sorted|ascending")
    c = cos.copy(); c[3] += np.float32(1e-3)
    add("a cosine off by 1e-3", c, ids, match="cos of id 500")
    c, i = cos.copy(), ids.copy(); c[9], i[9] = 0.0, NO_ID
    add("a short count", c, i, n=9, match="count 9, expected")
    add("a long count", c20, i20, n=11, match="count 11, expected")
    i = ids.copy(); i[9] = i[8]
    add("an id twice", cos, i, match="returned twice")
    add("an answer shorter than k", cos, ids, n=k, kk=12, allowed=ids.tolist(), match="shorter than k")
    few = ids[:5].tolist()
    c, i, n = m.topk(q, k, allowed=few)
    assert n == 5
    i[7] = 123
    add("a tail that is not empty slots", c, i, n=5, allowed=few, match="tail behind count")
    # a higher-id duplicate in place of the lower one: 351 returned, 350 left out (cosines equal: the order holds)
    # (at the end of the list, where the cosines alone cannot tell: only rule (f) sees it)
    add("a higher-id duplicate in place of a lower one", cos[:2], ids[[0, 2]], n=2, kk=2, match="lower id 350 is left out")
    # capped: the best of a group replaced by a worse member of the same group
    gc, gi, gn = m.topk(q, k, per_file=1)
    assert gn == k and gi[0] == 170 and m.check(q, k, (gc, gi, gn), per_file=1) <= 1e-7
    mate = next(x for x in range(int(gi[5]) + 1, int(gi[5]) + 16) if m.groups.get(x) == m.groups[int(gi[5])] and m.is_live(x))
    c, i = gc.copy(), gi.copy()
    c[5], i[5] = m.cosines(q)[np.searchsorted(m.live_ids(), mate)], mate
    order = np.lexsort((i, -c))
    add("a group's second best in place of its best", c[order], i[order], per_file=1, match="left out")
    return out


def test_the_judge_accepts_right_answers(little):
    m, rows, q = little
    for k in (1, 10, 200, 600):
        for per_file in (None, 1, 3):
            got = m.topk(q, k, per_file=per_file)
            assert m.check(q, k, got, per_file=per_file) <= 1e-7
        half = list(range(50, 650, 2))
        assert m.check(q, k, m.topk(q, k, allowed=half), allowed=half) <= 1e-7
        assert m.check(q, k, m.topk(q, k, allowed=[]), allowed=[]) == 0.0
    assert m.topk(q, 600)[2] == 539 and m.topk(q, 600, per_file=1)[2] == len({(i - 50) // 16 for i in m.live_ids().tolist()})
    # variants: an id scores its best over the queries
    qs = np.stack([q, rows[400], np.zeros(384, np.float32)])
    got = m.topk(qs, 5)
    assert got[1][:5].tolist() == [450, 170, 350, 351, 500] and m.check(qs, 5, got) <= 1e-7
    # ungrouped ids are never capped
    m2 = StoreModel(384)
    m2.insert(rows[:40])
    m2.set_groups(range(0, 20), [7] * 20)
    m2.set_groups([3], [NO_GROUP])
    m2.build()
    assert m2.groups_assigned() == 19 and m2.topk(q, 40, per_file=2)[2] == 21 + 2
    with pytest.raises(ValueError, match="never issued"):
        m2.set_groups([40], [1])


def test_the_judge_rejects_each_wrong_answer(little):
    m, rows, q = little
    cases = _mutations(m, q)
    assert len(cases) >= 12
    for name, k, got, allowed, per_file, match in cases:
        with pytest.raises(AssertionError, match=match):
            m.check(q, k, got, allowed=allowed, per_file=per_file)
            pytest.fail(f"the judge accepted: {name}")


def test_a_search_before_the_build_is_an_error(little):
    m = StoreModel(8)
    m.insert(np.ones((3, 8), np.float32))
    with pytest.raises(AssertionError, match=NOT_BUILT):
        m.check(np.ones(8, np.float32), 1, (np.zeros(1), np.zeros(1), 0))
    with pytest.raises(AssertionError, match=NOT_BUILT):
        m.topk(np.ones(8, np.float32), 1)


def test_the_model_follows_the_life_cycle():
    """Ids are never reused, the reclaim rule predicts the stored rows, clear restarts the ids, a reopening returns to
    the last build minus the deletes since."""
    m = StoreModel(4, id_base=10)
    rows = np.arange(400, dtype=np.float32).reshape(100, 4) + 1
    assert m.insert(rows[:50]) == list(range(10, 60)) and not m.built
    m.build()
    assert m.delete([10, 11, 12, 13]) == 4 and not m.built           # 8 %: tombstones
    assert not m.build() and (m.stored_rows(), len(m)) == (50, 46)
    assert m.delete([14]) == 1 and m.build() and (m.stored_rows(), len(m)) == (45, 45)   # 10 %: reclaimed
    assert m.delete([10, 14, 9, 60]) == 0 and m.built                # reclaimed, never issued, below id_base: nothing changes
    assert m.delete(m.live_ids()) == 45 and m.build() and m.stored_rows() == 0 and m.next_id == 60
    assert m.insert(rows[50:60]) == list(range(60, 70))              # the emptied index goes on counting
    m.set_groups([10, 65], [1, 2])                                   # a deleted id is accepted
    assert m.groups_assigned() == 2
    assert m.insert(rows[60:70]) == list(range(70, 80)) and m.delete([75]) == 1
    m.reopen()                                                       # back to the build: 60 ids, all of them removed
    assert (m.next_id, m.stored_rows(), len(m), m.built, m.groups_assigned()) == (60, 0, 0, True, 0)
    m.insert(rows[:5])
    m.build()
    m.clear()
    assert (m.next_id, m.stored_rows(), m.built, m.removed, m.groups) == (10, 0, False, set(), {})
    m.reopen()                                                       # clear removed the files
    assert (m.next_id, m.built) == (10, False)
    # a sharded store reclaims shard by shard
    s = StoreModel(4, shards=3, stripe=4)
    s.insert(rows[:36])
    s.build()
    assert s.delete([0, 1, 2, 3]) == 4                               # a third of shard 0, a ninth of the store
    assert s.build() and s.stored_rows() == 32 and s.compacted == [True, False, False]


@pytest.mark.parametrize("seed,dim,sharded", WALKS)
def test_every_walk_reaches_every_state(seed, dim, sharded):
    walk = make_walk(seed, dim, sharded)
    assert walk == make_walk(seed, dim, sharded)                     # deterministic
    assert 35 <= len(walk) - 1 <= 55
    cov = walk_coverage(walk)
    missing = sorted(k for k in required_coverage(walk) if not cov[k])
    assert not missing, missing
    m = new_model(walk)
    peak = 0
    for op in walk[1:]:
        apply(op, resolve(op, m), m)
        peak = max(peak, m.stored_rows())
    assert peak <= 3400
    if not sharded:
        assert peak > 3072 + 128                                     # past phase 0 of the filter by a whole int8 tile
        assert {f"up_{e}_by_append" for e in EDGES} <= set(cov)


def test_some_walk_has_a_non_zero_id_base():
    assert any(make_walk(s, d, sh)[0]["id_base"] for s, d, sh in WALKS)


# ======================================================================================================
# The kinds that start from stored rows (similar, pairs, clusters) and the boosted search
# ======================================================================================================

from codesearch_amd.search import boost_order, clusters_of_pairs, drop_excluded, pairs_above  # noqa: E402

SIMILAR_WALKS = [(s, 384) for s in range(4)] + [(s, 100) for s in range(2)]  # tests/test_gpu_store_walk_similar.py runs these
TABLE = np.array([1, 1.15, 0.5, 0, 1.01], np.float32)
B = float(BOUND)
# rows of the fixture below (id = row + 50): (source, clone, target cosine); file = row // 16
NEAR = {"0.999": (140, 141, 0.999), "0.97": (152, 400, 0.97), "+5e-4": (160, 420, B + 5e-4), "+2e-4": (170, 171, B + 2e-4),
        "-2e-4": (180, 440, B - 2e-4), "-5e-4": (190, 460, B - 5e-4), "0.85": (210, 480, 0.85), "dead end": (150, 410, 0.95)}
CHAIN_ROWS = (220, 230, 500)


def _clone_model(cut_middle=False):
    dim = 384
    rows = synth_rows(41, 0, 600, dim)
    rows[300], rows[301], rows[450] = rows[120], rows[120], rows[120]   # ids 170 = 350 = 351 = 500
    rows[130] = 0.0
    for a, b, t in NEAR.values():
        plant(rows, a, b, t)
    plant(rows, CHAIN_ROWS[0], CHAIN_ROWS[1], CHAIN)
    plant(rows, CHAIN_ROWS[1], CHAIN_ROWS[2], CHAIN)
    m = StoreModel(dim, id_base=50)
    ids = m.insert(rows)
    m.set_groups(ids, [(i - 50) // 16 for i in ids])
    m.set_classes(ids, [NO_CLASS if (i - 50) % 7 == 6 else (i - 50) % 5 for i in ids])
    m.build()
    assert m.delete(range(50, 110)) == 60
    assert m.build() and m.stored_rows() == 540
    assert m.delete([200] + ([50 + CHAIN_ROWS[1]] if cut_middle else [])) == 1 + cut_middle
    assert not m.build()
    return m, rows


@pytest.fixture(scope="module")
def clones():
    """`little` with planted near-copies (NEAR), a chain, classes and groups; ids 50..109 reclaimed, id 200 (the source of
    the "dead end" clone) a tombstone."""
    return _clone_model()


def _pid(name):
    a, b, _ = NEAR[name]
    return a + 50, b + 50


def _full_order(m, q):
    c, i, n = m.topk(q, len(m))
    assert n == len(m)
    return c, i


def test_planting_hits_its_targets(clones):
    m, rows = clones
    ids = m.live_ids()
    g = m._gram()
    at = lambda i: int(np.searchsorted(ids, i))
    for name, (a, b, t) in NEAR.items():
        if name != "dead end":
            assert abs(g[at(a + 50), at(b + 50)] - t) < 1e-6, name
    a, b, c = (r + 50 for r in CHAIN_ROWS)
    assert g[at(a), at(b)] > B + 0.02 and g[at(b), at(c)] > B + 0.02 and 0.8 < g[at(a), at(c)] < B - 0.02
    assert m.ambiguous_pairs(BOUND) == 0 and m.classes_assigned() == 600 - 600 // 7
    with pytest.raises(ValueError, match="never issued"):
        m.set_classes([650], [1])
    assert m.classes_assigned() == 600 - 600 // 7


def test_the_similar_judge_accepts_right_answers(clones):
    m, rows = clones
    grp = lambda ids: [m.groups.get(int(i), NO_GROUP) for i in ids]
    E = list(range(50, 700, 2))
    for src in (190, 191, 110, 649, 170, 500, 280, 180):  # a source, its clone, the ends, duplicates, the chain's middle, the zero row
        if src == 180:
            assert not m.rows[src].any()
        bound = m.pick_min_cos(src) if src != 180 else None
        fc, fi = _full_order(m, m.rows[src])
        for mode in ("none", "self", "file"):
            for k in (1, 10, 200, 600):
                for min_cos in (None, bound):
                    for allowed in (None, E):
                        got = m.similar_topk(src, k, mode, min_cos, allowed)
                        assert m.check_similar(src, k, got, mode, min_cos, allowed) <= 1e-7
                        keep = np.ones(len(fi), bool) if allowed is None else np.isin(fi, E)
                        hc, hi = drop_excluded(fc[keep], fi[keep], grp(fi[keep]), src, m.groups.get(src, NO_GROUP), mode,
                                               None if min_cos is None else np.float32(min_cos), k)
                        assert hi == got[1][:got[2]].tolist()   # the project's host statement agrees with the model
                        assert m.check_similar(src, k, _padded(hc, hi, k), mode, min_cos, allowed) <= 1e-7
    assert m.similar_topk(190, 3, "none")[1][:2].tolist() == [190, 191] and m.similar_topk(190, 3, "file")[1][0] != 191
    assert 0.5 < m.pick_min_cos(190) < 0.95


def test_the_similar_judge_rejects_each_wrong_answer(clones):
    m, rows = clones
    k = 10
    src = 190
    cases = []
    c, i, n = m.similar_topk(src, k, "none")
    cases.append(("the source under self", "self", None, (c, i, n), "source id 190 is returned under exclude='self'"))
    c, i, n = m.similar_topk(src, k, "self")
    assert i[0] == 191 and m.groups[191] == m.groups[190]
    cases.append(("a group-mate under file", "file", None, (c, i, n), "id 191 of the source's group 8 is returned"))
    bound = m.pick_min_cos(src)
    c2, i2, n2 = m.similar_topk(src, k, "self", bound)
    assert n2 == 1
    cases.append(("a row at or below min_cos", "self", bound, (c, i, 2), "is not above min_cos"))
    for bad, text in ((60, "id 60 was deleted and reclaimed"), (200, "id 200 is deleted")):
        j = i.copy(); j[9] = bad
        cases.append((text, "self", None, (c, j, n), text))
    cc, j = c.copy(), i.copy(); cc[9], j[9] = 0.0, NO_ID
    cases.append(("a short count", "self", None, (cc, j, 9), "count 9, expected"))
    for name, mode, min_cos, got, match in cases:
        with pytest.raises(AssertionError, match=match):
            m.check_similar(src, k, got, mode, min_cos)
            pytest.fail(f"the judge accepted: {name}")
    # a bound float64 cannot place is refused, not judged
    near = float(m.cosines(m.rows[src])[np.searchsorted(m.live_ids(), 191)])
    with pytest.raises(AssertionError, match="refused.*float64 cannot decide"):
        m.check_similar(src, k, (c, i, n), "self", near + 1e-5)
    with pytest.raises(AssertionError, match="source id 200 is deleted"):
        m.check_similar(200, k, (c, i, n), "self")


def _host_pairs(m, bound, other_files, max_pairs=65536):
    orders = {int(a): _full_order(m, m.rows[int(a)]) for a in m.live_ids()}
    return pairs_above(orders, lambda ids: [m.groups.get(int(i), NO_GROUP) for i in ids], "other_group" if other_files else "all",
                       bound, max_pairs)


def test_the_pairs_judge_accepts_right_answers(clones):
    m, rows = clones
    E, O = list(range(50, 700, 2)), list(range(51, 700, 2))
    full = m.pairs(BOUND, False)
    got = set(zip(full[1].tolist(), full[2].tolist()))
    want = {_pid(n) for n in ("0.999", "0.97", "+5e-4", "+2e-4")} | {(270, 280), (280, 550)} | \
        {(170, 350), (170, 351), (170, 500), (350, 351), (350, 500), (351, 500)}
    assert got == want and full[3] == 12
    for other_files in (False, True):
        for kw in ({}, {"max_pairs": 5}, {"inside": E}, {"inside": E, "other": O}, {"inside": O, "other": O}):
            ans = m.pairs(BOUND, other_files, **kw)
            assert m.check_pairs(BOUND, other_files, ans, **kw) <= 1e-7
        host = _host_pairs(m, BOUND, other_files)
        mine = m.pairs(BOUND, other_files)
        assert host[3] == mine[3] and host[1] == mine[1].tolist() and host[2] == mine[2].tolist()
        assert m.check_pairs(BOUND, other_files, host) <= 1e-7
        cut = _host_pairs(m, BOUND, other_files, 5)
        assert len(cut[0]) == 5 and m.check_pairs(BOUND, other_files, cut, max_pairs=5) <= 1e-7
    same_file = {(190, 191), (220, 221), (350, 351)}
    assert got - set(zip(*[x.tolist() for x in m.pairs(BOUND, True)[1:3]])) == same_file
    between = m.pairs(BOUND, False, inside=E, other=O)
    assert all((a % 2) != (b % 2) for a, b in zip(between[1].tolist(), between[2].tolist())) and 0 < between[3] < 12
    # no bound: every live pair once, the zero row's pairs at 0.0, nothing that is not finite
    small = StoreModel(384)
    small.insert(rows[120:135])
    small.build()
    every = small.pairs(None, False)
    assert every[3] == 15 * 14 // 2 and np.isfinite(every[0]).all() and (every[0][(every[1] == 10) | (every[2] == 10)] == 0).all()
    assert small.check_pairs(None, False, every) <= 1e-7
    assert small.check_pairs(None, False, _host_pairs(small, None, False)) <= 1e-7


def test_the_pairs_judge_rejects_each_wrong_answer(clones):
    m, rows = clones
    cos, a, b, total = m.pairs(BOUND, False)
    n = len(a)
    cases = []

    def add(name, match, c=cos, x=a, y=b, t=total, other_files=False, max_pairs=65536):
        cases.append((name, match, (np.asarray(c, np.float32), np.asarray(x, np.uint32), np.asarray(y, np.uint32), t), other_files, max_pairs))

    x, y = a.copy(), b.copy(); x[7], y[7] = b[7], a[7]
    add("a pair as (b, a)", "is not given as a < b", x=x, y=y)
    x, y, c = a.copy(), b.copy(), cos.copy(); x[8], y[8], c[8] = x[7], y[7], c[7]
    add("a pair twice", "is returned twice", c=c, x=x, y=y)
    oc, oa, ob, ot = m.pairs(BOUND, True)
    j = a.tolist().index(190)
    pos = int(np.searchsorted(-oc, -cos[j]))
    add("a same-group pair under other_files", r"pair \(190, 191\) lies inside group 8", c=np.insert(oc, pos, cos[j]),
        x=np.insert(oa, pos, 190), y=np.insert(ob, pos, 191), t=ot + 1, other_files=True)
    add("a same-group pair under other_files, total kept", r"pair \(190, 191\) lies inside group 8", c=np.insert(oc, pos, cos[j]),
        x=np.insert(oa, pos, 190), y=np.insert(ob, pos, 191), t=ot, other_files=True)
    dead = (200, 460)   # the 0.95 clone of the tombstoned id 200
    pos = int(np.searchsorted(-cos, -np.float32(0.95)))
    add("a pair with a deleted end", r"pair \(200, 460\): id 200 is deleted", c=np.insert(cos, pos, np.float32(0.95)),
        x=np.insert(a, pos, dead[0]), y=np.insert(b, pos, dead[1]), t=total + 1)
    lo = _pid("-2e-4")
    c_lo = np.float32(m._gram()[np.searchsorted(m.live_ids(), lo[0]), np.searchsorted(m.live_ids(), lo[1])])
    add("the pair at BOUND - 2e-4 present", r"pair \(230, 490\) is returned, but its float64 cos .* is not above the bound",
        c=np.append(cos, c_lo), x=np.append(a, lo[0]), y=np.append(b, lo[1]), t=total + 1)
    hi = _pid("+2e-4")
    keep = ~((a == hi[0]) & (b == hi[1]))
    assert keep.sum() == n - 1
    add("the pair at BOUND + 2e-4 missing", r"total 11, the model counts 12", c=cos[keep], x=a[keep], y=b[keep], t=total - 1)
    add("the pair at BOUND + 2e-4 missing, total kept", r"pairs returned, expected", c=cos[keep], x=a[keep], y=b[keep])
    add("a wrong total", "total 13, the model counts 12", t=total + 1)
    cut = [0, 1, 2, 3, 4, 5, 6, 8]   # the best seven, then the ninth in place of the eighth
    assert cos[7] > cos[8] + 2 * m.tol
    add("a cut list that drops a better pair", r"the cut list leaves out pair \(202, 450\)", c=cos[cut], x=a[cut], y=b[cut], max_pairs=8)
    c, x, y = cos.copy(), a.copy(), b.copy()
    assert cos[7] > cos[9]
    c[[7, 9]], x[[7, 9]], y[[7, 9]] = cos[[9, 7]], a[[9, 7]], b[[9, 7]]
    add("two entries swapped", "not sorted", c=c, x=x, y=y)
    c = cos.copy(); c[8] += np.float32(1e-3)
    add("a cosine off by 1e-3", "cos of pair", c=c)
    for name, match, got, other_files, max_pairs in cases:
        with pytest.raises(AssertionError, match=match):
            m.check_pairs(BOUND, other_files, got, max_pairs=max_pairs)
            pytest.fail(f"the judge accepted: {name}")
    # a pair float64 cannot place is refused, not judged
    with pytest.raises(AssertionError, match="refused.*float64 cannot decide"):
        m.check_pairs(np.float32(float(c_lo) + 1e-5), False, (cos, a, b, total))
    with pytest.raises(AssertionError, match="refused"):
        m.check_clusters(np.float32(float(c_lo) + 1e-5), False, *m.clusters(BOUND, False))


def test_the_clusters_judge(clones):
    m, rows = clones
    a_, b_, c_ = (r + 50 for r in CHAIN_ROWS)
    for other_files in (False, True):
        labels, clusters, members = m.clusters(BOUND, other_files)
        assert m.check_clusters(BOUND, other_files, labels, clusters, members) == 0.0
        pc, pa, pb, _ = m.pairs(BOUND, other_files)
        hl, hc, hm = clusters_of_pairs(m.live_ids(), pa, pb)   # the project's host statement agrees with the model
        host = np.full(len(labels), NO_ID, np.uint32)
        for i, root in hl.items():
            host[i - 50] = root
        assert host.tolist() == labels.tolist() and (hc, hm) == (clusters, members)
        assert m.check_clusters(BOUND, other_files, host, hc, hm) == 0.0
    labels, clusters, members = m.clusters(BOUND, False)
    assert labels[a_ - 50] == labels[b_ - 50] == labels[c_ - 50] == a_ and labels[500 - 50] == 170 and labels[200 - 50] == NO_ID
    assert (clusters, members) == (6, 2 * 4 + 3 + 4) and len(labels) == 600 and (labels[:60] == NO_ID).all()
    cases = []
    l = labels.copy(); l[[a_ - 50, b_ - 50, c_ - 50]] = b_
    cases.append(("a label that is not the smallest id", f"id {a_} carries label {b_}, the smallest id of its component is {a_}", l, clusters, members))
    l = labels.copy(); l[200 - 50] = 200
    cases.append(("a deleted id with a label", "id 200 is deleted and carries label 200, not NO_ID", l, clusters, members))
    l = labels.copy(); l[60 - 50] = 60
    cases.append(("a reclaimed id with a label", "id 60 was deleted and reclaimed and carries label 60", l, clusters, members))
    l = labels.copy(); l[300 - 50] = NO_ID
    cases.append(("a live id with NO_ID", "live id 300 carries NO_ID", l, clusters, members))
    l = labels.copy(); l[c_ - 50] = c_
    cases.append(("the chain's ends not joined", f"id {c_} carries label {c_}, the smallest id of its component is {a_}", l, clusters - 0, members - 1))
    cases.append(("labels shifted by one entry", "carries", np.roll(labels, 1), clusters, members))
    cases.append(("a wrong clusters", "clusters 7, the model counts 6", labels, clusters + 1, members))
    cases.append(("a wrong members", "members 14, the model counts 15", labels, clusters, members - 1))
    cases.append(("too few labels", "599 labels, expected", labels[:-1], clusters, members))
    for name, match, l, c, mm in cases:
        with pytest.raises(AssertionError, match=match):
            m.check_clusters(BOUND, False, l, c, mm)
            pytest.fail(f"the judge accepted: {name}")
    # the chain's middle deleted: the answer that still joins the ends is wrong there
    cut, _ = _clone_model(cut_middle=True)
    with pytest.raises(AssertionError, match=f"id {b_} is deleted and carries label|id {c_} carries label {a_}, the smallest id of its component is {c_}"):
        cut.check_clusters(BOUND, False, labels, clusters, members)
    l = labels.copy(); l[b_ - 50] = NO_ID
    with pytest.raises(AssertionError, match=f"id {c_} carries label {a_}, the smallest id of its component is {c_}"):
        cut.check_clusters(BOUND, False, l, clusters, members)
    assert cut.check_clusters(BOUND, False, *cut.clusters(BOUND, False)) == 0.0 and cut.clusters(BOUND, False)[1:] == (5, 12)


def _classes_of(m, ids):
    return [m.classes.get(int(i), NO_CLASS) for i in ids]


def test_the_boosted_judge_accepts_right_answers(clones):
    m, rows = clones
    q = (rows[120] + 0.3 * rows[20]).astype(np.float32)   # near the duplicates 170 = 350 = 351 = 500
    qs = np.stack([q, rows[400], synth_rows(43, 0, 1, 384)[0]])
    E = list(range(50, 700, 2))
    for weights in (TABLE, TABLE[:3], np.zeros(0, np.float32), None, np.ones(5, np.float32)):
        for k in (1, 10, 200, 600):
            for query in (q, qs[2], qs):
                for allowed in (None, E):
                    got = m.boosted_topk(query, k, weights, allowed)
                    assert m.check_boosted(query, k, got, weights, allowed) <= 1e-7
                    fc, fi = _full_order(m, query)
                    keep = np.ones(len(fi), bool) if allowed is None else np.isin(fi, E)
                    hs, hc, hi = boost_order(fc[keep], fi[keep], _classes_of(m, fi[keep]), weights, k)
                    assert hi.tolist() == got[2][:got[3]].tolist() and hs.tobytes() == got[0][:got[3]].tobytes()
                    pad = lambda x, fill, t: np.concatenate([x, np.full(k - len(x), fill, t)]).astype(t)
                    host = (pad(hs, 0, np.float32), pad(hc, 0, np.float32), pad(hi, NO_ID, np.uint32), len(hi))
                    assert m.check_boosted(query, k, host, weights, allowed) <= 1e-7
    plain = m.topk(q, 10)
    ones = m.boosted_topk(q, 10, np.ones(5, np.float32))
    assert ones[2].tolist() == plain[1].tolist() and ones[1].tobytes() == plain[0].tobytes()
    assert m.boosted_topk(q, 10, TABLE)[2].tolist() != plain[1].tolist()


def test_the_boosted_judge_rejects_each_wrong_answer(clones):
    m, rows = clones
    q = (rows[120] + 0.3 * rows[20]).astype(np.float32)
    k = 10
    score, cos, ids, cnt = m.boosted_topk(q, k, TABLE)
    assert cnt == k
    w = m._weights(TABLE)[np.searchsorted(m.live_ids(), ids)]
    assert len(set(w.tolist())) >= 2
    cases = []

    def add(name, match, s=score, c=cos, i=ids, n=cnt, weights=TABLE, kk=k, query=q):
        cases.append((name, match, (np.asarray(s, np.float32), np.asarray(c, np.float32), np.asarray(i, np.uint32), n), weights, kk, query))

    j = int(np.flatnonzero(w != np.float32(1.15))[0])
    s = score.copy(); s[j] = m.score_of(cos[j], np.float32(1.15))
    add("the cosine's score times the wrong class's weight", f"score of id {ids[j]} is", s=s)
    # a score rounded twice: the reference's two successive multiplies where the table holds f32(1.2 * 1.15)
    both = np.array([np.float32(1.2) * np.float32(1.15)] * 5, np.float32)
    s2, c2, i2, n2 = m.boosted_topk(q, 200, both)
    classed = m._weights(both)[np.searchsorted(m.live_ids(), i2)] != 1   # (an id without a class weighs 1 either way)
    twice = np.where(classed, (m.score_of(c2, np.float32(1.15)) * np.float32(1.2)).astype(np.float32), s2)
    assert (twice != s2).any() and np.abs(twice - s2).max() < 2e-7
    add("a score rounded twice", "score of id", s=twice, c=c2, i=i2, n=n2, weights=both, kk=200)
    full = m.boosted_topk(q, k + 1, TABLE)
    drop = int(np.flatnonzero(w > 1)[0])
    keep = [n for n in range(k + 1) if n != drop]
    assert full[0][drop] > full[0][k] + 1e-4
    add("a boosted row left out", f"id {ids[drop]} .* is left out", s=full[0][keep], c=full[1][keep], i=full[2][keep])
    by_cos = np.lexsort((ids, -cos))
    assert by_cos.tolist() != list(range(k))
    add("order by cosine instead of score", "not sorted by", s=score[by_cos], c=cos[by_cos], i=ids[by_cos])
    pc, pi, pn = m.topk(q, k)
    assert pi.tolist() != sorted(ids.tolist(), key=ids.tolist().index)
    add("the plain top-k with scores attached", "is left out|not sorted by", c=pc, i=pi,
        s=m.score_of(pc, m._weights(TABLE)[np.searchsorted(m.live_ids(), pi)]))
    # weight 0: every row of class 3 scores 0.0; among them the order is the id's
    zero = np.array([0, 0, 0, 0, 0], np.float32)
    zs, zc, zi, zn = m.boosted_topk(q, 600, zero)
    tied = np.flatnonzero(zs[:zn] == 0)
    assert len(tied) > 300 and (np.diff(zi[tied].astype(np.int64)) > 0).all()
    zi2, zc2 = zi.copy(), zc.copy()
    zi2[tied], zc2[tied] = zi[tied][::-1], zc[tied][::-1]
    add("a weight-0 tie in descending id", "not sorted by", s=zs, c=zc2, i=zi2, n=zn, weights=zero, kk=600)
    i = ids.copy(); i[9] = 200
    add("a deleted id", "id 200 is deleted", i=i)
    add("a short count", "count 9, expected", s=np.append(score[:9], 0), c=np.append(cos[:9], 0), i=np.append(ids[:9], NO_ID), n=9)
    # byte-identical rows of one class: 170 and 500 both carry class 0 (351 class 1, 350 none); 500 in place of 170 at the
    # end of a list, where the scores alone cannot tell
    assert m.classes[170] == m.classes[500] == 0 and m.classes[351] == 1 and 350 not in m.classes
    dq = rows[120]
    ds, dc, di, dn = m.boosted_topk(dq, 2, TABLE)
    assert di.tolist() == [351, 170]
    add("a higher-id duplicate of the same class in place of a lower one", "lower id 170 .* is left out", s=ds, c=dc,
        i=np.array([351, 500]), n=2, kk=2, query=dq)
    for name, match, got, weights, kk, query in cases:
        with pytest.raises(AssertionError, match=match):
            m.check_boosted(query, kk, got, weights)
            pytest.fail(f"the judge accepted: {name}")


def test_the_default_walks_are_unchanged():
    import hashlib

    for seed, dim, sharded in WALKS:
        walk = make_walk(seed, dim, sharded)
        assert walk == make_walk(seed, dim, sharded, extended=False)
        assert not any(op["op"] == "classes" or "clones" in op for op in walk)
        ext = make_walk(seed, dim, sharded, extended=True)
        plain = [{k: v for k, v in op.items() if k != "clones"} for op in ext if op["op"] != "classes"]
        assert plain == walk                                         # the same operations, order, sizes and seeds
        assert sum(op["op"] == "classes" for op in ext) == sum(op["op"] == "groups" for op in ext)
        assert all(("clones" in op) == (op["n"] >= 64) for op in ext if op["op"] == "insert")
    # an insert without the key gives the rows it gave before the key existed (synth_rows, dups, zero and nothing else)
    op = {"op": "insert", "n": 300, "seed": 7001, "first": 90, "dups": 3, "zero": True}
    rows = synth_rows(7001, 90, 300, 384)
    rows[297:] = rows[:3]
    rows[1] = 0.0
    assert rows_of(op, 384).tobytes() == rows.tobytes()
    assert hashlib.sha256(rows_of(op, 384).tobytes()).hexdigest() == hashlib.sha256(rows.tobytes()).hexdigest()
    cloned = rows_of(dict(op, clones=8101), 384)
    changed = np.flatnonzero((cloned != rows).any(axis=1)).tolist()
    plants, chains = clone_layout(dict(op, clones=8101))
    assert changed == sorted(b for _, b, _ in plants) and len(changed) == len(LADDER) + 2
    assert not set(changed) & {0, 1, 2, 297, 298, 299} and not set(changed) & {a for a, _, _ in plants if a not in {c[1] for c in chains}}
    assert np.allclose(np.linalg.norm(cloned[changed], axis=1), np.linalg.norm(rows[changed], axis=1), rtol=1e-6)
    near = [abs(a - b) for a, b, _ in plants]
    assert sum(d <= 16 for d in near) >= 2 and sum(d > 16 for d in near) >= 2


@pytest.mark.parametrize("seed,dim", SIMILAR_WALKS)
def test_every_extended_walk_reaches_every_state(seed, dim):
    walk = make_walk(seed, dim, False, extended=True)
    cov = walk_coverage(walk)
    missing = sorted(k for k in required_coverage(walk) if not cov[k])
    assert not missing, missing
    ext = extended_coverage(walk)
    assert ext["ambiguous"] == 0 and ext["min_cos_failed"] == 0, ext     # the ambiguity cap: zero
    assert ext["classes_before_reclaim"] >= 1 and ext["appended_after_classes"] >= 1, ext
    if dim == 384:  # (the pairs and clusters calls have no tiles for another dim)
        assert ext["full_states"] >= 6 and ext["chain_cut"] >= 1, ext
    assert any(make_walk(s, d, False, True)[0]["id_base"] for s, d in SIMILAR_WALKS) and \
        any(not make_walk(s, d, False, True)[0]["id_base"] for s, d in SIMILAR_WALKS)
