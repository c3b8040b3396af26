"""Pins tests/store_model.py on the CPU: the model's bookkeeping, its judge against the C oracle's answers — and against
hand-made WRONG answers, each of which it must reject: a judge that accepts everything is the failure this file guards
against — and the coverage of every walk the GPU test runs (tests/test_gpu_store_walk.py)."""
import json
import os

import numpy as np
import pytest

from codesearch_amd.synth import synth_planted, synth_rows
from tests.store_model import (EDGES, NO_GROUP, NO_ID, NOT_BUILT, WALKS, StoreModel, apply, make_walk, new_model,
                               required_coverage, resolve, tolerance, walk_coverage)

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
