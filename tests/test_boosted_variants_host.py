"""Host side of the boosted variants searches, no GPU: the contract as host Python (search.merge_variants_boosted: the GPU
tests' ground truth) against a brute-force statement of it — dicts and Python floats rounded through np.float32 — over a
few thousand small random universes, with and without the per-file cap; the three identities of the contract at the host
level; the ABI additions (declared, exported, bound; cs_abi_version stays 6) and vector_store._filters_ok's new
allowance."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from codesearch_amd.search import boost_order, merge_variants_boosted
from codesearch_amd.vector_store import NO_CLASS, NO_GROUP, _filters_ok

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cs_index_search_variants_boosted", "cs_index_search_variants_boosted_scoped",
       "cs_index_search_variants_boosted_grouped", "cs_index_search_variants_boosted_grouped_scoped"]
f32 = np.float32


def _r(x):
    """A Python float rounded through np.float32."""
    return float(f32(x))


def _brute(lists, classes, weights, k, groups=None, m=None):
    """The contract, sentence by sentence.  lists: [(cos, ids)]; classes / groups: {id: value} -> [(b, c, id)], best first."""
    best = {}
    for cos, ids in lists:
        for c, i in zip(cos, ids):
            c, i = float(c), int(i)
            if i not in best or c > best[i]:
                best[i] = c                                   # c = max_v c_v
    rows = []
    for i, c in best.items():
        s = _r(1.0 - _r(_r(1.0 - c) * 0.5))                    # s = 1.0f - (1.0f - c) * 0.5f
        cls = classes.get(i, NO_CLASS)
        w = float(weights[cls]) if cls < len(weights) else 1.0  # weights[class] for a class below n_classes, else 1
        rows.append((_r(s * w), c, i))                         # b = s * w with one rounding
    rows.sort(key=lambda r: (-r[0], r[2]))                     # key order: b descending, then id ascending
    kept, have = [], {}
    for b, c, i in rows:
        if len(kept) >= k:
            break
        g = NO_GROUP if groups is None else groups.get(i, NO_GROUP)
        if m is not None and g != NO_GROUP:
            if have.get(g, 0) >= m:
                continue
            have[g] = have.get(g, 0) + 1
        kept.append((b, c, i))
    return kept


def _universe(rng):
    """At most 40 rows, 4 variants, 5 groups, 4 classes; cosines on a grid of eighths and weights from a short menu that
    holds 0, so b ties often; some ids without class or group; a table that may be shorter than the classes."""
    n = int(rng.integers(1, 41))
    ids = np.sort(rng.choice(200, n, replace=False)).astype(np.uint32)
    nv = int(rng.integers(1, 5))
    lists = []
    for _ in range(nv):
        cos = (rng.integers(-8, 9, n) / 8.0).astype(f32)
        if rng.random() < 0.5:
            cos = (cos + rng.integers(-2, 3, n) * f32(2.0 ** -20)).astype(f32).clip(-1, 1)  # and near-ties that round apart
        order = np.lexsort((ids, -cos))
        lists.append((cos[order], ids[order]))
    classes = {int(i): int(rng.integers(0, 4)) for i in ids if rng.random() < 0.8}
    groups = {int(i): int(rng.integers(0, 5)) for i in ids if rng.random() < 0.8}
    weights = rng.choice(np.array([0.0, 0.5, 1.0, 1.15, 1.25, 2.0], f32), int(rng.integers(0, 5))).astype(f32)
    return ids, lists, classes, groups, weights


def _lookup(table, none):
    return lambda ids: [table.get(int(i), none) for i in ids]


def _same(got, want):
    b, c, i = got
    assert b.dtype == f32 and c.dtype == f32 and i.dtype == np.uint32
    assert i.tolist() == [r[2] for r in want]
    assert b.tobytes() == np.array([r[0] for r in want], f32).tobytes()
    assert c.tobytes() == np.array([r[1] for r in want], f32).tobytes()


def test_merge_variants_boosted_is_the_contract():
    rng = np.random.default_rng(20260)
    ties = capped_differs = 0
    for _ in range(3000):
        ids, lists, classes, groups, weights = _universe(rng)
        class_of, group_of = _lookup(classes, NO_CLASS), _lookup(groups, NO_GROUP)
        k = int(rng.integers(1, 45))
        m = int(rng.integers(1, 5))
        plain = _brute(lists, classes, weights, k)
        _same(merge_variants_boosted(lists, class_of, weights, k), plain)
        capped = _brute(lists, classes, weights, k, groups, m)
        _same(merge_variants_boosted(lists, class_of, weights, k, group_of, m), capped)
        ties += len({r[0] for r in plain}) < len(plain)
        capped_differs += [r[2] for r in capped] != [r[2] for r in plain]
        # the identities: a cap that cannot bind, or no group at all, is the uncapped answer
        _same(merge_variants_boosted(lists, class_of, weights, k, group_of, k), plain)
        _same(merge_variants_boosted(lists, class_of, weights, k, _lookup({}, NO_GROUP), m), plain)
        # one variant, uncapped: the boosted search of that variant's list
        one = boost_order(lists[0][0], lists[0][1], class_of(lists[0][1]), weights, k)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(merge_variants_boosted(lists[:1], class_of, weights, k), one))
        # a scope is a restriction of the rows in play: one that holds every id changes nothing, a real one is the
        # contract over the rows inside
        inside = ids[rng.random(ids.size) < 0.5]
        for sub in (ids, inside):
            cut = [(c[np.isin(i, sub)], i[np.isin(i, sub)]) for c, i in lists]
            _same(merge_variants_boosted(cut, class_of, weights, k, group_of, m),
                  _brute(cut, classes, weights, k, groups, m) if sub is inside else capped)
    assert ties > 1000 and capped_differs > 1000  # the universes exercise what they are meant to


def test_merge_variants_boosted_edges():
    none = _lookup({}, NO_CLASS)
    b, c, i = merge_variants_boosted([], none, None, 5)
    assert b.size == c.size == i.size == 0
    b, c, i = merge_variants_boosted([(np.zeros(0, f32), np.zeros(0, np.uint32))], none, None, 5, _lookup({}, NO_GROUP), 1)
    assert i.size == 0
    # a chunk's cosine is its best over the variants, and so is its boosted score
    lists = [(np.array([0.5, 0.25], f32), np.array([1, 2], np.uint32)), (np.array([0.75, 0.0], f32), np.array([2, 1], np.uint32))]
    b, c, i = merge_variants_boosted(lists, _lookup({1: 0}, NO_CLASS), np.array([1.25], f32), 5)
    assert i.tolist() == [1, 2] and c.tolist() == [0.5, 0.75] and b.tolist() == [0.9375, 0.875]
    # the cap walks b, not the cosine: file 7 keeps its boosted chunk, not its nearest
    b, c, i = merge_variants_boosted(lists, _lookup({1: 0}, NO_CLASS), np.array([1.25], f32), 5, _lookup({1: 7, 2: 7}, NO_GROUP), 1)
    assert i.tolist() == [1]


def _declared():
    text = open(os.path.join(ROOT, "include", "codesearch_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_abi_additions(gpu_lib):
    from codesearch_amd import _lib

    hdr = _declared()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name + " is not declared"
        assert hasattr(raw, name) and re.search(r"\b" + name + r"$", exported, re.M), name + " is not exported"
        assert name in _lib.SIGNATURES
        args = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        assert len(_lib.SIGNATURES[name][1]) == len([a for a in args.split(",") if a.strip()]), name
    assert gpu_lib.cs_abi_version() == 6  # additions only


def test_variants_may_combine_class_weights_with_per_file():
    w = np.ones(3, f32)
    _filters_ok(None, None, 2, w, variants=True)
    _filters_ok(None, object(), 2, w, variants=True)
    _filters_ok(None, object(), None, w, variants=True)
    with pytest.raises(ValueError, match="class_weights= is exclusive with chunk_ids="):
        _filters_ok([1], None, None, w, variants=True)
    with pytest.raises(ValueError, match="per_file= is exclusive with chunk_ids="):
        _filters_ok([1], None, 2, None, variants=True)
    with pytest.raises(ValueError, match="class_weights= is exclusive with per_file="):
        _filters_ok(None, None, 2, w)  # independent queries: as before
