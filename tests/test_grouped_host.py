"""Host side of the grouped search, no GPU: the C++ plan and selection rule (codesearch_amd/csrc/grouped_plan.hpp) through
tests/cpp/grouped_plan_test.cpp, the contract as host Python (search.cap_per_group: the GPU tests' ground truth) on
hand-made cases, and search.group_results_by_file against the reference's display order under `--per-file`
(src/search/mod.rs:1007-1038)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from codesearch_amd.search import NO_GROUP, cap_per_group, group_results_by_file
from codesearch_amd.vector_store import SearchResult

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "grouped_plan_test.cpp")


def test_grouped_plan_cpp():
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "grouped_plan_test")
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "grouped plan ok" in r.stdout


def _cap(rows, k, m):
    """rows: (cos, id, group) already in (cosine desc, id asc) order -> kept ids."""
    cos, ids, groups = zip(*rows) if rows else ((), (), ())
    kc, ki = cap_per_group(cos, ids, groups, k, m)
    assert kc == [cos[ids.index(i)] for i in ki]
    return ki


def test_cap_per_group_contract():
    rows = [(0.9, 4, 7), (0.8, 1, 7), (0.8, 2, 7), (0.7, 9, 3), (0.6, 0, NO_GROUP), (0.5, 5, 7), (0.4, 6, NO_GROUP),
            (0.3, 8, 3), (0.2, 3, 2)]
    assert _cap(rows, 10, 1) == [4, 9, 0, 6, 3]          # one row per group, ungrouped rows never capped
    assert _cap(rows, 10, 2) == [4, 1, 9, 0, 6, 8, 3]    # a tie inside a group: the lower id takes the m-th slot
    assert _cap(rows, 3, 2) == [4, 1, 9]                 # stop at k
    assert _cap(rows, 2, 2) == [4, 1]                    # ... a tie at the k-th slot: the lower id
    assert _cap(rows, 4, 4) == [4, 1, 2, 9]              # m >= k: the plain top-k
    assert _cap(rows, 9, 9) == [r[1] for r in rows]
    assert _cap(rows, 5, 100) == [4, 1, 2, 9, 0]
    # fewer groups than needed: the count is what the cap leaves
    two = [(1.0 - i / 100, i, i % 2) for i in range(50)]
    assert _cap(two, 10, 1) == [0, 1]
    assert _cap(two, 10, 3) == [0, 1, 2, 3, 4, 5]
    # no groups at all
    none = [(1.0 - i / 100, i, NO_GROUP) for i in range(50)]
    assert _cap(none, 10, 1) == list(range(10))
    assert _cap([], 10, 1) == []
    # numpy inputs, as the GPU tests pass them
    kc, ki = cap_per_group(np.array([0.5, 0.4, 0.3], np.float32), np.array([7, 8, 9], np.uint32),
                           np.array([1, 1, NO_GROUP], np.uint32), 5, 1)
    assert ki == [7, 9] and np.asarray(kc, np.float32).tobytes() == np.array([0.5, 0.3], np.float32).tobytes()


def _res(i, path, score):
    return SearchResult(id=i, content="", path=path, start_line=1, end_line=2, kind="Function", signature=None,
                        docstring=None, context=None, hash="", distance=1.0 - score, score=score)


def _reference_order(results, per_file):
    """mod.rs:1010-1038 step by step: group by path, order the files by the maximum of 0.0 and their scores, sort each
    file's hits by score, truncate."""
    by_file = {}
    for r in results:
        by_file.setdefault(r.path, []).append(r)
    files = list(by_file.items())
    files.sort(key=lambda kv: -max(0.0, *[r.score for r in kv[1]]))
    out = []
    for _path, rs in files:
        rs = sorted(rs, key=lambda r: -r.score)
        out += rs[:per_file]
    return out


def test_group_results_by_file_is_the_reference_order():
    rs = [_res(0, "a.rs", 0.90), _res(1, "b.rs", 0.85), _res(2, "a.rs", 0.80), _res(3, "c.rs", 0.75), _res(4, "b.rs", 0.95),
          _res(5, "a.rs", 0.70), _res(6, "d.rs", -0.2)]
    got = group_results_by_file(rs, 2)
    assert [r.id for r in got] == [4, 1, 0, 2, 3, 6]      # b.rs first: its best hit leads; a.rs cut to two
    assert [r.id for r in group_results_by_file(rs, 1)] == [4, 0, 3, 6]
    rng = np.random.default_rng(3)
    for _ in range(50):
        n = int(rng.integers(1, 40))
        scores = rng.permutation(n) / n - 0.1  # distinct, some negative
        many = [_res(i, "f%d.rs" % rng.integers(0, 6), float(scores[i])) for i in range(n)]
        for per_file in (1, 2, 5):
            assert [r.id for r in group_results_by_file(many, per_file)] == [r.id for r in _reference_order(many, per_file)]
    # mod.rs:1008-1009, :1039-1044: no cap, a cap of 0, or one not below max_results leaves the list as it is
    assert group_results_by_file(rs, None) == rs
    assert group_results_by_file(rs, 0) == rs
    assert group_results_by_file(rs, 10, max_results=10) == rs
    assert [r.id for r in group_results_by_file(rs, 2, max_results=10)] == [4, 1, 0, 2, 3, 6]


def test_per_file_is_exclusive_with_masks_and_scopes():
    from codesearch_amd.vector_store import _one_of

    _one_of(None, None, 3)
    _one_of([1], None, None)
    with pytest.raises(ValueError, match="exclusive"):
        _one_of([1], None, 3)
    with pytest.raises(ValueError, match="exclusive"):
        _one_of(None, object(), 1)
